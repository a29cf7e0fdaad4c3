"""Velocity commands on the GPU (include/solorl.h solorl_commands / solorl_shape_reward_cmd; solorl_amd/command.py and
SoloVecEnv(commands=)).  The kernel against the host program (csrc/command.hpp compiled alone by g++) and the Python prediction of
tests/command_util.py, bitwise; then twin handles: commands add three observation words and change nothing else; the tracking terms
against each row's own command; capture, the refusals, joystick control, reset_masked, PPO with --commands and eval_ppo.py --command."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from solorl_amd import _native, command
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from tests import command_util as cu
from tests.host_util import build_host
from tests.test_command_host import FIXED, WALK, obs_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SEED, OFF = 2301, 2 ** 32 - 40     # (the larger batches straddle the 32-bit boundary of the global env id)
CALLS = 12
WALK_DICT = dict(lin_vel_x=(WALK.lo[0], WALK.hi[0]), lin_vel_y=(WALK.lo[1], WALK.hi[1]), yaw_rate=(WALK.lo[2], WALK.hi[2]), interval=WALK.interval,
                 zero_prob=WALK.zero_prob, min_lin_norm=WALK.min_lin_norm, obs_scale=WALK.obs_scale)


@pytest.fixture(scope="module")
def exe():
    return build_host("command_main")


def _params(D, p=WALK, seed=SEED, off=OFF):
    return command.make_params(seed, off, D, lin_vel_x=(p.lo[0], p.hi[0]), lin_vel_y=(p.lo[1], p.hi[1]), yaw_rate=(p.lo[2], p.hi[2]), interval=p.interval,
                               zero_prob=p.zero_prob, min_lin_norm=p.min_lin_norm, obs_scale=p.obs_scale)


def _view(n, W, offset_words, fill=0.0):
    """[n, W] float32 view that starts offset_words floats into its (16-byte aligned) buffer"""
    buf = torch.full((n * W + 4,), fill, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[offset_words:offset_words + n * W].view(n, W)


def _restarts(n):
    """flags of the 12 calls: call 0 and most others pass NULL, three calls restart every fifth env (shifted by the call)"""
    return ["".join("1" if (i + t) % 5 == 0 else "0" for i in range(n)) if t in (3, 4, 9) else "-" for t in range(CALLS)]


def _flag_tensor(s):
    return None if s == "-" else torch.tensor([c == "1" for c in s], dtype=torch.uint8, device=DEV)


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


#                 obs_in offset, obs_out offset (floats)    read path
ALIGNMENTS = [(0, 0), (0, 1), (1, 0)]                     # 16-byte words, 16-byte words, word by word


@pytest.mark.parametrize("off_in,off_out", ALIGNMENTS)
@pytest.mark.parametrize("D", (42, 76, 84))
@pytest.mark.parametrize("n", (1, 63, 130))
def test_kernel_equals_the_host_program_and_the_prediction(gpu_device, exe, n, D, off_in, off_out):
    """12 consecutive calls over zeroed memory with restarts: mem, cmd_out and obs_out after every call, bit for bit"""
    p = _params(D)
    flags = _restarts(n)
    obs = obs_rows(CALLS, n, D)
    h_rows, h_cmd, h_out = cu.host_commands(exe, SEED, OFF, n, D, WALK, flags, ["-"] * CALLS, obs)
    ref = cu.Commands(SEED, OFF, n, WALK)
    mem = command.CommandMem(n, DEV)
    src, dst = _view(n, D, off_in), _view(n, D + 3, off_out, fill=7.0)
    assert (src.data_ptr() % 16 == 0) == (off_in == 0) and (dst.data_ptr() % 16 == 0) == (off_out == 0)
    cmd_out = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    drew = 0
    for t in range(CALLS):
        src.copy_(torch.from_numpy(obs[t]))
        got = command.commands(p, mem, src, out=dst, cmd_out=cmd_out, restart=_flag_tensor(flags[t]))
        assert got.data_ptr() == dst.data_ptr()
        d, want = ref.call(None if flags[t] == "-" else [c == "1" for c in flags[t]], None, obs[t])
        drew += int(d.sum())
        rows = _u32(mem.data).reshape(n, 8)
        assert np.array_equal(rows, ref.rows()) and np.array_equal(rows, h_rows[t]), (n, D, t)
        assert np.array_equal(_u32(dst), want.view(np.uint32)) and np.array_equal(_u32(dst), h_out[t]), (n, D, t)
        assert np.array_equal(np.ascontiguousarray(cmd_out.cpu().numpy()).view(np.uint64), h_cmd[t]), (n, D, t)
        assert np.array_equal(_u32(src), obs[t].view(np.uint32))                         # the input is never written
    assert drew >= 3 * n                                                                 # 12 calls at 2..5 steps between draws, and the restarts


def test_masked_rows_and_their_memory_are_untouched(gpu_device):
    """n = 130, D = 76: every third row masked, and of the second workgroup's 64 rows all but one (a wavefront with one live lane)"""
    n, D = 130, 76
    p = _params(D)
    mask = np.arange(n) % 3 != 1
    mask[64:128] = False
    mask[70] = True
    ref = cu.Commands(SEED, OFF, n, WALK)
    mem = command.CommandMem(n, DEV)
    obs = obs_rows(3, n, D)
    src = torch.from_numpy(obs[0]).to(DEV)
    command.commands(p, mem, src, cmd_out=None)                                          # every env has drawn once
    ref.call(None, None, obs[0])
    poison = torch.full((n, 4), float("nan"), dtype=torch.float64, device=DEV)
    m = torch.from_numpy(mask).to(DEV)
    mem.data[~m] = poison[~m]                                                            # the masked rows' memory: a pattern any write would change
    before = _u32(mem.data).reshape(n, 8).copy()
    src = torch.from_numpy(obs[1]).to(DEV)
    src[~m] = float("nan")
    out = torch.full((n, D + 3), 7.0, dtype=torch.float32, device=DEV)
    cmd_out = torch.full((n, 3), 7.0, dtype=torch.float64, device=DEV)
    restart = torch.ones(n, dtype=torch.uint8, device=DEV)                               # ... a restart flag does not reach a masked row either
    command.commands(p, mem, src, out=out, cmd_out=cmd_out, restart=restart, mask=m)
    _, want = ref.call(np.ones(n, bool), mask, obs[1])
    rows = _u32(mem.data).reshape(n, 8)
    assert np.array_equal(rows[mask], ref.rows()[mask]) and np.array_equal(rows[~mask], before[~mask])
    assert np.array_equal(_u32(out)[mask], want.view(np.uint32)[mask]) and bool((out[~m] == 7.0).all())
    assert np.array_equal(cmd_out.cpu().numpy()[mask], ref.cmd[mask]) and bool((cmd_out[~m] == 7.0).all())
    assert np.all(ref.draws[mask] == 2)


def test_the_no_observation_form_writes_mem_and_cmd_out_only(gpu_device, exe):
    n = 130
    p = _params(76)
    flags = _restarts(n)
    h_rows, h_cmd, _ = cu.host_commands(exe, SEED, OFF, n, 0, WALK, flags, ["-"] * CALLS, None)
    ref = cu.Commands(SEED, OFF, n, WALK)
    mem = command.CommandMem(n, DEV)
    cmd_out = torch.zeros((n, 3), dtype=torch.float64, device=DEV)
    for t in range(CALLS):
        assert command.commands(p, mem, cmd_out=cmd_out, restart=_flag_tensor(flags[t])) is None
        ref.call(None if flags[t] == "-" else [c == "1" for c in flags[t]])
        assert np.array_equal(_u32(mem.data).reshape(n, 8), ref.rows()) and np.array_equal(ref.rows(), h_rows[t]), t
        assert np.array_equal(np.ascontiguousarray(cmd_out.cpu().numpy()).view(np.uint64), h_cmd[t]), t
    command.commands(p, mem)                                                             # cmd_out == NULL too: only the memory rows
    ref.call()
    assert np.array_equal(_u32(mem.data).reshape(n, 8), ref.rows())
    with pytest.raises(_native.SoloRLError, match="solorl_commands:"):                    # exactly one of obs_in / obs_out
        _native.check(_native.lib().solorl_commands(__import__("ctypes").byref(p), None, None, n, mem.data.data_ptr(), None,
                                                    cmd_out.data_ptr(), None, 0, None))


@pytest.mark.parametrize("D", (42, 76))
def test_two_shards_equal_one_batch(gpu_device, D):
    n = 130
    obs = obs_rows(CALLS, n, D)
    whole, a, b = (command.CommandMem(k, DEV) for k in (n, 65, 65))
    pw, pa, pb = _params(D), _params(D), _params(D, off=OFF + 65)
    for t in range(6):
        x = torch.from_numpy(obs[t]).to(DEV)
        r = torch.from_numpy((np.arange(n) + t) % 7 == 0).to(DEV) if t == 3 else None
        ow = command.commands(pw, whole, x, restart=r)
        oa = command.commands(pa, a, x[:65].contiguous(), restart=None if r is None else r[:65].contiguous())
        ob = command.commands(pb, b, x[65:].contiguous(), restart=None if r is None else r[65:].contiguous())
        assert np.array_equal(_u32(ow), _u32(torch.cat([oa, ob]))), t
    assert torch.equal(whole.data, torch.cat([a.data, b.data])) and not torch.equal(a.cmd, b.cmd)


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


def _same_info(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("N", (6, 130))
def test_commands_add_three_words_and_change_nothing_else(gpu_device, N):
    A, B = _env(N, commands=WALK_DICT), _env(N)
    D = B.obs_dim
    assert (A.engine_obs_dim, A.obs_dim, A.observation_space.shape, B.engine_obs_dim) == (D, D + 3, (D + 3,), D) and B.last_commands is None
    ref = cu.Commands(5, 3, N, WALK)
    oa, ob = A.reset(), B.reset()
    ref.call(np.ones(N, bool))
    assert torch.equal(oa[:, :D], ob) and np.array_equal(_u32(oa[:, D:]), ref.words().view(np.uint32))
    resets = 0
    for t, act in enumerate(_actions(N, 30)):
        if t % 2:
            (oa, ra, da, ia), (ob, rb, db, ib) = A.step_inplace(act), B.step_inplace(act)
        else:
            (oa, ra, da, la), (ob, rb, db, lb) = A.step(act), B.step(act)
            ia, ib = la.tensors, lb.tensors
        assert torch.equal(ra, rb) and torch.equal(da, db) and _same_info(ia, ib), t        # rewards, done flags and info: the plain twin's
        ref.call(db.cpu().numpy() != 0)                                                     # the twin's done flags are the restarts
        assert np.array_equal(_u32(oa[:, :D]), _u32(ob)), t
        assert np.array_equal(_u32(oa[:, D:]), ref.words().view(np.uint32)), t
        assert np.array_equal(A.last_commands.cpu().numpy(), ref.cmd), t
        resets += int(db.sum())
    assert resets >= 2 * N                                                                  # auto-resets occurred (episode_length 10)
    assert np.array_equal(A.get_states().bytes().cpu().numpy(), B.get_states().bytes().cpu().numpy())
    g = A.get_observation()
    assert torch.equal(g[:, :D], B.get_observation()) and np.array_equal(_u32(g[:, D:]), ref.words().view(np.uint32))
    assert np.array_equal(_u32(A._cmd_mem.data).reshape(N, 8), ref.rows())
    # reset_masked: the selected rows draw, no other row does; every row carries the command it holds
    mask = torch.arange(N, device=DEV) % 3 == 0
    before = ref.draws.copy()
    oa, ob = A.reset_masked(mask), B.reset_masked(mask)
    m = mask.cpu().numpy()
    ref.call(m, m)
    assert np.array_equal(ref.draws - before, m.astype(np.uint32))
    assert torch.equal(oa[:, :D], ob) and np.array_equal(_u32(oa[:, D:]), ref.words().view(np.uint32))
    assert np.array_equal(_u32(A._cmd_mem.data).reshape(N, 8), ref.rows())
    A.close(); B.close()


def test_tracking_terms_follow_each_rows_own_command(gpu_device):
    """solorl_shape_reward_cmd with rows against the tests/shape_util.py prediction evaluated with each row's own command, to the bound
    tests/test_shape_gpu.py holds every term to (shape_util.check_outputs: kin_util.TOL); with NULL it is solorl_shape_reward, bitwise"""
    from solorl_amd.shaping import ShapeMem, make_params, shape_reward
    from solorl_amd.state import StateBatch
    from tests import kin_util as ku, shape_util as su
    c = su.case(1, 65)                                        # (a case tests/test_shape_gpu.py uses: one more row than a workgroup takes)
    dev = lambda a: torch.tensor(np.array(a), device=DEV)
    rng = np.random.default_rng(3)
    cmds = command.CommandMem(c.n, DEV)
    cmd = rng.uniform(-1.0, 1.0, (c.n, 3))
    cmds.cmd.copy_(dev(cmd))
    cmds.countdown.fill_(-1)                                  # (only the cmd member is read)
    cmds.draws.fill_(-1)

    def call(commands):
        sb, mem = StateBatch(data=dev(c.states)), ShapeMem(data=dev(c.mem))
        reward, terms, ep = dev(c.reward), dev(c.terms), dev(c.ep)
        shape_reward(c.cfg, c.params, sb, dev(c.actions), dev(c.done), mem, reward, terms_out=terms, ep_out=ep, commands=commands)
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in (mem.data, reward, terms, ep))
    got = call(cmds)
    # the prediction: shape_util.reference on the case with the row's own command in the parameters, row by row
    weights = {name: c.params.weight[k] for k, name in enumerate(su.TERMS)}
    other = {k: getattr(c.params, k) for k in ("base_height_target", "foot_clearance_target", "foot_force_max", "air_time_target", "tracking_sigma")}
    want = [np.zeros_like(g) for g in got]
    for i in range(c.n):
        ci = types.SimpleNamespace(**vars(c))
        ci.params = make_params(weights, cmd_lin_vel=(cmd[i, 0], cmd[i, 1]), cmd_yaw_rate=cmd[i, 2], **other)
        (wm, wr, wt, we), _ = su.reference(ci, mask=np.arange(c.n) == i)
        want[0][i], want[1][i], want[2][i], want[3][:, i] = wm[i], wr[i], wt[i], we[:, i]
    su.check_outputs(c, got, tuple(want))
    live = c.done == 0
    assert ku.close(got[2][live][:, 14:], want[2][live][:, 14:], ku.TOL).all()
    plain = call(None)
    assert not np.allclose(got[2][live][:, 14:], plain[2][live][:, 14:])                  # (the rows' commands are not the parameters' one)
    # NULL rows: the existing call, bit for bit -- through the new entry point itself
    import ctypes as C
    sb, mem = StateBatch(data=dev(c.states)), ShapeMem(data=dev(c.mem))
    reward, terms, ep, actions, done = dev(c.reward), dev(c.terms), dev(c.ep), dev(c.actions), dev(c.done)
    _native.check(_native.lib().solorl_shape_reward_cmd(C.byref(c.cfg), C.byref(c.params), sb.data.data_ptr(), None, c.n, actions.data_ptr(), done.data_ptr(),
                                                        mem.data.data_ptr(), reward.data_ptr(), terms.data_ptr(), ep.data_ptr(), None, 0, None))
    torch.cuda.synchronize()
    null = tuple(x.cpu().numpy() for x in (mem.data, reward, terms, ep))
    assert all(np.array_equal(su.bits(a), su.bits(b)) for a, b in zip(null, plain))


WEIGHTS = {"lin_vel_z": -2.0, "action_rate": -0.01, "foot_slip": -0.1, "tracking_lin_vel": 1.0, "tracking_yaw_rate": 0.5}
GROUPS = {"height": 0.01, "orientation": 0.03, "lin_vel": 0.1, "ang_vel": 0.2, "joint_pos": 0.01, "joint_vel": 1.5}


def test_a_captured_step_with_commands_shaping_and_noise_equals_an_eager_twin(gpu_device):
    N = 130
    A, B = _env(N, commands=WALK_DICT), _env(N, commands=WALK_DICT)
    for e in (A, B):
        e.set_reward_shaping(WEIGHTS)
        e.set_obs_noise(GROUPS)                           # (both allocate here: before the capture)
        e.reset()
    act = torch.zeros(N, 12, device=DEV)
    acts = _actions(N, 9, seed=21)
    act.copy_(acts[0])
    oa, ra, da, _ = A.step_inplace(act)                   # a warm-up step on both
    ob, rb, db, _ = B.step_inplace(acts[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa, ra, da, _ = A.step_inplace(act)
    shaped = 0
    for r in range(8):
        act.copy_(acts[1 + r])
        graph.replay()
        ob, rb, db, _ = B.step_inplace(acts[1 + r])
        torch.cuda.synchronize()
        assert oa.shape == (N, A.engine_obs_dim + 3) and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), r
        assert torch.equal(A._cmd_mem.data, B._cmd_mem.data) and torch.equal(A._noise_count, B._noise_count)
        assert torch.equal(A.last_shaping_terms, B.last_shaping_terms) and torch.equal(A._shape_mem.data, B._shape_mem.data)
        shaped += int((A.last_shaping_terms[:, 14] != 0).sum())
    assert shaped > 4 * N and int(A._cmd_mem.draws.min()) >= 2
    assert np.array_equal(A.get_states().bytes().cpu().numpy(), B.get_states().bytes().cpu().numpy())
    assert len(torch.unique(A.last_commands[:, 0])) > N // 2          # (the envs hold commands of their own)
    A.close(); B.close()


def test_refusals_joystick_control_and_the_off_state(gpu_device):
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import Box, make_vec_envs
    N = 8
    plain = _env(N)
    assert all(getattr(plain, k) is None for k in ("_cmd", "_cmd_mem", "_cmd_all")) and plain._obs_engine is plain._obs     # off: nothing is allocated
    with pytest.raises(_native.SoloRLError, match="set_command_ranges"):
        plain.set_command_ranges(interval=1)
    torch.manual_seed(3)
    P = policy_params(Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(DEV))
    assert plain.step_act_supported(P) and plain.rollout_supported(P)
    plain.close()
    env = _env(N, commands=WALK_DICT)
    assert not env.step_act_supported(P) and not env.rollout_supported(P)
    env.reset()
    acts = torch.zeros(2, N, 12, device=DEV)
    val, lp = torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV)
    with pytest.raises(_native.SoloRLError, match="step_n.*velocity commands"):
        env.step_n_inplace(acts)
    with pytest.raises(_native.SoloRLError, match="step_n.*velocity commands"):
        env.step_n(acts)
    with pytest.raises(_native.SoloRLError, match="rollout_inplace.*velocity commands"):
        env.rollout_inplace(acts, P, None, val, lp)
    with pytest.raises(_native.SoloRLError, match="step_act_inplace.*velocity commands"):
        env.step_act_inplace(acts[0], P, None, val[0], acts[1], lp[0])
    with pytest.raises(AssertionError):
        env.step_inplace(acts[0], obs_out=torch.zeros(N, 76, device=DEV))               # the caller's rows are the wide ones
    with pytest.raises(ValueError, match="heading"):
        env.set_command_ranges(heading=(0.0, 1.0))
    # joystick control: lo == hi and an interval of 1 -- every env holds exactly that command after one step
    env.set_command_ranges(lin_vel_x=0.3, lin_vel_y=(-0.1, -0.1), yaw_rate=0.7, interval=1, zero_prob=0.0, min_lin_norm=0.0)
    wide = torch.zeros(N, 79, device=DEV)
    o, _, _, _ = env.step_inplace(acts[0], obs_out=wide)
    assert o.data_ptr() == wide.data_ptr()
    assert np.array_equal(env.last_commands.cpu().numpy(), np.tile(np.array(FIXED.lo), (N, 1)))
    scale = np.array(WALK.obs_scale)
    assert np.array_equal(wide[:, 76:].cpu().numpy(), np.tile((np.array(FIXED.lo) * scale).astype(np.float32), (N, 1)))     # obs_scale stayed
    env.close()
    made = make_vec_envs(dict(episode_length=10, solo12=True, task="walk", num_history_stack=1), N, device=DEV, commands=WALK_DICT, norm_obs=True)
    assert made.obs_dim == 79 and tuple(made.ob_rms.mean.shape) == (79,) and made.reset().shape == (N, 79)
    made.close()


# ---- training and evaluation with the flags
T_STEPS, N_TRAIN, UPDATES = 16, 64, 2


def _train(monkeypatch, graphs):
    """train() for two updates of 64 walk12 envs x 16 steps with --commands, shaping and noise -> (the env, the GraphedRollout or None, the history)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd import vec_env
    from solorl_amd.ppo import train as tr
    from solorl_amd.config import load_yaml
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N_TRAIN), "--num-steps", str(T_STEPS),
            "--num-env-steps", str(N_TRAIN * T_STEPS * UPDATES), "--mini-batch-size", "512", "--ppo-epoch", "2", "--use-gae", "--seed", "7", "--log-interval", "1",
            "--commands", os.path.join(ROOT, "configs", "commands_walk12.yaml"), "--reward-shaping", os.path.join(ROOT, "configs", "shaping_walk12.yaml"),
            "--obs-noise", os.path.join(ROOT, "configs", "noise_solo.yaml")]
    if not graphs:
        argv += ["--no-hip-graphs"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    args.obs_noise = train_ppo.load_obs_noise(args.obs_noise, config)
    args.commands = train_ppo.load_commands(args.commands)
    args.reward_shaping = load_yaml(args.reward_shaping)
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
    return seen["env"], seen.get("graphed"), hist, pol


@pytest.mark.parametrize("graphs", (True, False), ids=("hip_graphs", "eager"))
def test_training_with_commands(gpu_device, monkeypatch, graphs):
    monkeypatch.setenv("SOLORL_ROLLOUT_CHUNK", "8")         # falls back to one launch per step by itself
    env, graphed, hist, pol = _train(monkeypatch, graphs)
    for rec in hist:
        assert all(math.isfinite(float(rec[k])) for k in rec if "loss" in k or k == "entropy"), rec
        assert any("loss" in k for k in rec), rec
    if graphs:
        assert graphed is not None and graphed.graph is not None and graphed.step_act is False and graphed.windows is None
    else:
        assert graphed is None
    D = env.engine_obs_dim
    assert env.obs_dim == D + 3 and pol.base.features[0].in_features == D + 3
    # reset() and every rollout step went through solorl_commands: every env has drawn, and the noise count says how many calls there were
    assert int(env._cmd_mem.draws.min()) >= 1 and np.all(env._noise_count.cpu().numpy() == 1 + UPDATES * T_STEPS)
    c = env.last_commands.cpu().numpy()
    assert np.all(np.abs(c[:, 0]) <= 1.0) and np.all(np.abs(c[:, 1]) <= 0.3) and len(np.unique(c[:, 2])) > N_TRAIN // 2
    assert env._shape_params is not None and float(env._shape_mem.ep_sum.abs().sum()) > 0.0


def test_eval_ppo_with_a_fixed_command(gpu_device, tmp_path, capsys):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval_ppo
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(5)
    pol = Policy((79,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64})
    torch.save({"update": 0, "state_dict": pol.state_dict(), "ob_rms": None}, os.path.join(str(tmp_path), "solo.pt"))
    base = ["--checkpoint-dir", str(tmp_path), "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", "16",
            "--num-runs", "4", "--max-steps", "60", "--deterministic"]
    r = eval_ppo.main(base + ["--command", "0.3", "0", "0"])
    out = capsys.readouterr().out
    assert "command tracking over" in out and "mean |v_b.xy - cmd.xy|" in out
    assert math.isfinite(r["tracking_error_lin_vel"]) and math.isfinite(r["tracking_error_yaw_rate"])
    assert 0.0 < r["tracking_error_lin_vel"] < 5.0 and 0.0 <= r["tracking_error_yaw_rate"] < 50.0     # (an untrained policy: it tracks nothing)
    r2 = eval_ppo.main(base + ["--commands", os.path.join(ROOT, "configs", "commands_walk12.yaml")])
    assert math.isfinite(r2["tracking_error_lin_vel"]) and r2 != r
    with pytest.raises(SystemExit, match="79.*76|76.*79"):                              # the checkpoint's width against the flags', both named
        eval_ppo.main(base)
