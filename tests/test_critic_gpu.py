"""solorl_critic_obs on the GPU: the kernel on the rows of a real engine after 20 random steps against the numpy word table of
tests/critic_util.py (whose docstring says which words are held bit for bit and which to the kinematics rows' tolerance) -- 130 envs,
two workgroups and a ragged third, both robots, with a mask, with every block NULL and with all blocks present -- and the stage in
SoloVecEnv beside every other stage: the rows against the table on what the env holds, the actor's side bitwise that of an env without
the stage, a captured graph against eager steps, and the refused paths."""
import numpy as np
import pytest
import torch

from solorl_amd import _native
from solorl_amd.channel import ActuatorMem
from solorl_amd.command import CommandMem
from solorl_amd.config import ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK, default_config
from solorl_amd.critic_obs import CRITIC_PRIV, critic_obs, make_params
from tests import critic_util as cu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 130
CASES = {"solo12_walk": (ROBOT_SOLO12, TASK_WALK), "solo8_stand": (ROBOT_SOLO8, TASK_STAND)}


def _actions(n, A, steps, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return [(torch.rand(n, A, device=DEV, generator=g) * 2 - 1).contiguous() for _ in range(steps)]


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", params=sorted(CASES))
def engine_rows(request, gpu_device):
    """(cfg, params, the state rows of 130 envs after 20 random steps, their clean observation rows with two NaNs and a -0.0 put in,
    random command, actuator and kick rows, the 0xA5 fill, the kinematics host rows of the states): computed once per robot"""
    from solorl_amd.vec_env import SoloVecEnv
    robot, task = CASES[request.param]
    cfg = default_config(robot, task)
    cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N, device=DEV, seed=5)
    env.reset()
    for a in _actions(N, env.act_dim, 20):
        env.step_inplace(a)
    states = env.get_states()
    obs = env.get_observation().clone()
    E = env.engine_obs_dim
    env.close()
    obs.view(torch.int32)[2, E - 1] = 0x7FC12345
    obs.view(torch.int32)[3, 0] = -0x005FFFFF              # 0xFFA00001: a signalling NaN, negative
    obs[4, E // 2] = -0.0
    c = cu.case(robot, n=N, E=E)                            # (its command, actuator and kick rows and its fill; its states are not used)
    rows = _np(states.data)
    assert len(np.unique(cu.su.contact_masks(rows) & 0xFFFFFF)) > 4 and cu.timesteps(rows).max() > 0
    return cfg, make_params(cfg, E), states, obs, c, cu.kin_rows(cfg, rows)


def _call(cfg, params, states, obs, c, flags=cu.F_ALL, mask=None):
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)           # (a copy: the case's arrays are read-only)
    out = dev(c.fill)
    got = critic_obs(cfg, params, states, obs, out=out, commands=CommandMem(data=dev(c.cmd)) if flags & cu.F_CMD else None,
                     actuators=ActuatorMem(data=dev(c.act)) if flags & cu.F_ACT else None, kick=dev(c.kick) if flags & cu.F_KICK else None,
                     mask=None if mask is None else dev(mask))
    torch.cuda.synchronize()
    assert got is out
    return _np(out)


def _want(cfg, params, states, obs, c, kin, flags=cu.F_ALL, mask=None):
    return cu.reference(cfg, cu.scale_of(params), _np(states.data), _np(obs), c.fill, c.cmd if flags & cu.F_CMD else None,
                        c.act if flags & cu.F_ACT else None, c.kick if flags & cu.F_KICK else None, mask, kin=kin)


@pytest.mark.parametrize("flags", (cu.F_ALL, 0, cu.F_CMD, cu.F_ACT | cu.F_KICK), ids=("all", "none", "cmd", "act_kick"))
def test_kernel_against_the_word_table(engine_rows, flags):
    cfg, params, states, obs, c, kin = engine_rows
    got = _call(cfg, params, states, obs, c, flags)
    want, raw = _want(cfg, params, states, obs, c, kin, flags)
    E = params.obs_dim
    print("feet words: max |got - want| = %.3e" % np.abs(got[:, E:E + 12].astype(np.float64) - want[:, E:E + 12]).max())
    cu.check(got, want, raw, cu.scale_of(params), E)
    assert cu.bits(got)[2, E - 1] == 0x7FC12345 and cu.bits(got)[3, 0] == 0xFFA00001 and cu.bits(got)[4, E // 2] == 0x80000000


def test_kernel_with_a_mask(engine_rows):
    """masked rows keep the fill's bytes; their inputs (NaN states and observations here) are not read"""
    cfg, params, states, obs, c, kin = engine_rows
    mask = (np.arange(N) % 3 != 1).astype(np.uint8) * 7
    off = torch.from_numpy(mask == 0).to(DEV)
    bad_states, bad_obs = states.clone(), obs.clone()
    bad_states.data[off] = float("nan")
    bad_obs[off] = float("nan")
    got = _call(cfg, params, bad_states, bad_obs, c, mask=mask)
    want, raw = _want(cfg, params, states, obs, c, kin, mask=mask)
    cu.check(got, want, raw, cu.scale_of(params), params.obs_dim, mask=mask)
    assert (cu.bits(got)[mask == 0] == 0xA5A5A5A5).all()


# ---------------------------------------------------------------- the stage in SoloVecEnv
def _env(critic, n=64, seed=9):
    from solorl_amd.vec_env import SoloVecEnv
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1
    cfg.episode_length = 12
    env = SoloVecEnv(cfg, n, device=DEV, seed=seed, commands={"lin_vel_x": [-0.5, 1.0], "lin_vel_y": [-0.3, 0.3], "yaw_rate": [-1.0, 1.0], "interval": [3, 6]},
                     critic_obs=critic)
    env.set_perturbation((2, 4), 0.5, 0.3)
    env.set_actuation((0, 3), 0.2)
    env.set_termination(max_tilt_deg=50, contacts=["base"], min_steps=1)
    env.set_obs_noise(dict(height=0.01, orientation=0.02, lin_vel=0.05, ang_vel=0.1, joint_pos=0.01, joint_vel=0.5))
    env.set_reset_randomization(joint_pos=0.2, joint_vel=1.0, yaw=3.14, roll=0.1, pitch=0.1)
    return env


def _check_rows(env, what):
    """last_critic_obs against get_observation() and the table on what the env holds now"""
    torch.cuda.synchronize()
    E = env.engine_obs_dim
    got = _np(env.last_critic_obs)
    clean = _np(env.get_observation())
    assert clean.shape[1] == E + 3 and (cu.bits(got)[:, :E] == cu.bits(clean)[:, :E]).all(), what
    rows = _np(env.get_states().data)
    cmd = np.zeros((env.nenvs, cu.CMD_WORDS))
    cmd[:, :3] = _np(env.last_commands)
    want, raw = cu.reference(env.cfg, cu.scale_of(env._critic), rows, clean[:, :E].copy(), got, cmd, _np(env._act_mem.data), _np(env.last_kick))
    cu.check(got, want, raw, cu.scale_of(env._critic), E)
    return raw


def test_stage_beside_every_other_stage(gpu_device):
    n = 64
    env, twin = _env(dict(foot_force=0.1, command=[2.0, 2.0, 0.25]), n), _env(None, n)
    assert env.critic_obs_dim == env.engine_obs_dim + CRITIC_PRIV == 96 and env.critic_observation_space.shape == (96,)
    assert env.obs_dim == twin.obs_dim == 79 and tuple(env.last_critic_obs.shape) == (n, 96)
    assert twin.critic_obs_dim is None and twin.last_critic_obs is None and twin._critic is None and twin._critic_clean is None     # off: nothing is allocated
    assert list(env._critic.scale[12:15]) == [2.0, 2.0, 0.25] and env._critic.scale[0] == 0.1
    assert torch.equal(env.reset().view(torch.int32), twin.reset().view(torch.int32))
    _check_rows(env, "reset")
    seen = np.zeros(CRITIC_PRIV, bool)
    finished = 0
    for t, a in enumerate(_actions(n, 12, 30)):
        o, r, d, _ = env.step_inplace(a)
        o2, r2, d2, _ = twin.step_inplace(a)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int32), o2.view(torch.int32)) and torch.equal(r.view(torch.int32), r2.view(torch.int32)) and torch.equal(d, d2), t
        finished += int(d.sum())
        if t % 5 in (0, 3):
            assert not torch.equal(env._obs_engine.view(torch.int32), env._critic_clean.view(torch.int32)), "the actor's rows carry the noise"
            seen |= (_check_rows(env, t) != 0).any(axis=0)       # (get_observation() inside refills the engine's buffer: after the line above)
    # every privileged word but the collision count was non-zero at some checked step (a collision of a knee or a shoulder is not
    # forced here: word 16 is covered by the kernel tests above, whose rows hold some)
    assert finished >= 2 * n and np.delete(seen, 16).all(), (finished, seen)
    assert torch.equal(env.get_states().bytes(), twin.get_states().bytes())
    # caller-owned rows, reset_masked, and the refused paths
    mine = torch.zeros(n, 96, device=DEV)
    env.step_inplace(a, critic_obs_out=mine)
    twin.step_inplace(a)
    keep = env.last_critic_obs.clone()
    got, env.last_critic_obs = env.last_critic_obs, mine
    _check_rows(env, "critic_obs_out")
    env.last_critic_obs = got
    assert torch.equal(got.view(torch.int32), keep.view(torch.int32)), "last_critic_obs is not written when the caller gives rows"
    mask = torch.arange(n, device=DEV) % 3 == 0
    assert torch.equal(env.reset_masked(mask).view(torch.int32), twin.reset_masked(mask).view(torch.int32))
    _check_rows(env, "reset_masked")
    with pytest.raises(AssertionError, match="^critic_obs_out must be "):
        env.step_inplace(a, critic_obs_out=torch.zeros(n, 95, device=DEV))
    with pytest.raises(_native.SoloRLError, match="critic_obs_out on an env made without critic_obs"):
        twin.step_inplace(a, critic_obs_out=mine)
    env.close(); twin.close()


def test_refused_paths_and_construction(gpu_device):
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import Box, SoloVecEnv, make_vec_envs
    n = 8
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1
    torch.manual_seed(3)
    P = policy_params(Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(DEV))
    plain, env = SoloVecEnv(cfg, n, device=DEV, seed=2), SoloVecEnv(cfg, n, device=DEV, seed=2, critic_obs=True)
    assert plain.step_act_supported(P) and plain.rollout_supported(P)
    assert not env.step_act_supported(P) and not env.rollout_supported(P)
    assert torch.equal(plain.reset().view(torch.int32), env.reset().view(torch.int32))
    acts = torch.zeros(2, n, 12, device=DEV)
    val, lp = torch.zeros(2, n, device=DEV), torch.zeros(2, n, device=DEV)
    with pytest.raises(_native.SoloRLError, match="step_n with critic_obs"):
        env.step_n_inplace(acts)
    with pytest.raises(_native.SoloRLError, match="step_n with critic_obs"):
        env.step_n(acts)
    with pytest.raises(_native.SoloRLError, match="rollout_inplace with critic_obs"):
        env.rollout_inplace(acts, P, None, val, lp)
    with pytest.raises(_native.SoloRLError, match="step_act_inplace with critic_obs(.|\n)*value from the actor's row"):
        env.step_act_inplace(acts[0], P, None, val[0], acts[1], lp[0])
    # no optional stage: the engine's rows are the clean rows, every optional block is NULL, and the actor's side is the plain env's
    for t, a in enumerate(_actions(n, 12, 5, seed=4)):
        (o1, r1, d1, _), (o2, r2, d2, _) = plain.step_inplace(a), env.step_inplace(a)
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(d1, d2), t
        assert torch.equal(env.last_critic_obs[:, :76].view(torch.int32), o2.view(torch.int32)), t
    tail = env.last_critic_obs[:, 76:]
    ts = _np(env.get_states().timestep).astype(np.float64)
    assert not bool(tail[:, 12:15].any()) and not bool(tail[:, 17:].any()) and ts.max() == 5
    assert (_np(tail[:, 15]) == (ts * (1.0 / cfg.episode_length)).astype(np.float32)).all()
    plain.close(); env.close()
    with pytest.raises(_native.SoloRLError, match="critic_obs on an env with norm_obs"):
        SoloVecEnv(cfg, n, device=DEV, norm_obs=True, critic_obs=True)
    with pytest.raises(ValueError, match="foot_farce"):
        SoloVecEnv(cfg, n, device=DEV, critic_obs={"foot_farce": 1.0})
    config = dict(episode_length=10, solo12=True, task="walk", num_history_stack=1)
    made = make_vec_envs(config, n, device=DEV, critic_obs={"kick": 3.0}, norm_ret=True)
    assert made.critic_obs_dim == 96 and made._critic.scale[19] == 3.0 and made._critic.scale[15] == 0.1
    made.close()


def test_captured_steps_equal_eager_ones(gpu_device):
    n = 64
    A, B = _env(True, n, seed=4), _env(True, n, seed=4)
    assert torch.equal(A.reset().view(torch.int32), B.reset().view(torch.int32))
    acts = _actions(n, 12, 3 + 6, seed=21)
    for a in acts[:3]:                                   # (a warm-up: every engine-owned buffer exists before the capture)
        A.step_inplace(a); B.step_inplace(a)
    act = [torch.zeros(n, 12, device=DEV) for _ in range(3)]
    out = [(torch.zeros(n, A.obs_dim, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
            torch.zeros(n, A.critic_obs_dim, device=DEV)) for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(3):
            A.step_inplace(act[k], obs_out=out[k][0], rew_out=out[k][1], done_out=out[k][2], critic_obs_out=out[k][3])
    for r in range(2):
        for k in range(3):
            act[k].copy_(acts[3 + 3 * r + k])
        graph.replay()
        for k in range(3):
            ob, rb, db, _ = B.step_inplace(acts[3 + 3 * r + k])
            torch.cuda.synchronize()
            assert torch.equal(out[k][0].view(torch.int32), ob.view(torch.int32)) and torch.equal(out[k][1].view(torch.int32), rb.view(torch.int32)), (r, k)
            assert torch.equal(out[k][2], db), (r, k)
            assert torch.equal(out[k][3].view(torch.int32), B.last_critic_obs.view(torch.int32)), (r, k)
        assert torch.equal(A.get_states().bytes(), B.get_states().bytes()), r
    A.close(); B.close()


@pytest.mark.parametrize("applied_torque", (False, True), ids=("plain", "applied_torque"))
def test_rows_the_shaped_terms_read_are_reused(gpu_device, applied_torque, monkeypatch):
    """With reward shaping set and neither a termination nor a reset randomization the stage takes the rows the shaped terms have read
    in this step (with applied_torque their tau is overwritten first: the critic reads no tau) -- no get_states of its own -- and the
    rows still equal the table on a fresh get_states()"""
    from solorl_amd.vec_env import SoloVecEnv
    n = 64
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1
    cfg.episode_length = 6                               # (the engine's auto-reset inside the step: the rows are read behind it)
    env = SoloVecEnv(cfg, n, device=DEV, seed=7, applied_torque=applied_torque, critic_obs=True)
    env.set_reward_shaping({"foot_slip": -0.1, "torques": -0.01, "power": -0.01})
    env.set_perturbation((2, 4), 0.5, 0.3)
    env.reset()
    reads = []
    real = env.get_states
    monkeypatch.setattr(env, "get_states", lambda *a, **kw: (reads.append(kw.get("out")), real(*a, **kw))[1])
    finished = 0
    for t, a in enumerate(_actions(n, 12, 14, seed=5)):
        reads.clear()
        o, r, d, _ = env.step_inplace(a)
        assert len(reads) == 1 and reads[0] is env._shape_states, t       # one read per step, the shaped terms'
        finished += int(d.sum())
        if applied_torque:
            assert bool((env._shape_states.tau != 0).any())
        E = env.engine_obs_dim
        torch.cuda.synchronize()
        got = _np(env.last_critic_obs)
        rows = _np(real().data)
        assert (cu.bits(got)[:, :E] == cu.bits(_np(o))).all(), t          # (no noise: the actor's rows are the clean rows)
        want, raw = cu.reference(env.cfg, cu.scale_of(env._critic), rows, _np(o), got, None, None, _np(env.last_kick))
        cu.check(got, want, raw, cu.scale_of(env._critic), E)
    assert finished >= 2 * n
    env.close()
