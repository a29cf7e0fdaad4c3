"""Early termination on the GPU (include/solorl.h solorl_terminate; SoloVecEnv.set_termination).

1 the kernel against the header's table (tests/term_util.py, numpy) on the crafted rows of the host test, bit for bit, n = 6 and 130
  (ragged groups of four, more than one workgroup), with and without a mask, a poison fill in everything it must not touch;
2 a twin run against the engine's own fall rule: the engine with disable_termination and the rule base_height = 0.05 through
  solorl_terminate + solorl_reset_masked against the engine ending the same episodes itself, every output and state row after every step;
3 composition with shaping, actuation, commands and noise; 4 three captured steps against an eager twin; 5 the refused paths;
6 an env that set and cleared a termination against one that never had one; a short training run with --termination and eval_ppo.py --termination."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from solorl_amd import _native, termination
from solorl_amd.config import (EnvState, InfoSoA, PRECISION_F64, ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK, default_config)
from solorl_amd.state import StateBatch
from tests import term_util as tu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 130)


# ---- 1: the kernel against the table
def _cfg(robot12):
    c = default_config(ROBOT_SOLO12 if robot12 else ROBOT_SOLO8, TASK_WALK)
    assert c.sim_dt == tu.SIM_DT
    return c


def gpu_terminate(robot12, p, rows, arrays, mask=None, info=True, stats=True):
    """one solorl_terminate launch on device copies of ``arrays`` -> (the arrays after it, the rows after it)"""
    n = rows.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    sb = StateBatch(data=dev(rows))
    t = {k: dev(getattr(arrays, k)) for k in tu.Arrays.NAMES}
    soa = InfoSoA(timeout=t["timeout"].data_ptr(), success=t["success"].data_ptr(), episode_reward=t["ep_reward"].data_ptr(),
                  ep_stats=t["ep_stats"].data_ptr()) if info else None
    m = None if mask is None else dev(mask)
    out = termination.terminate(_cfg(robot12), p.struct(), sb, t["done"], t["reward"], t["fired"], info=soa, term_stats=t["stats"] if stats else None, mask=m)
    torch.cuda.synchronize()
    assert out is t["fired"]
    got = arrays.copy()
    for k in tu.Arrays.NAMES:
        setattr(got, k, t[k].cpu().numpy())
    return got, sb.data.cpu().numpy()


def _check(robot12, p, rows, done, reward, names, mask=None, info=True, stats=True, seed=0):
    before = tu.Arrays(rows.shape[0], done, reward, seed=seed)
    got, rows_after = gpu_terminate(robot12, p, rows, before, mask, info, stats)
    want = tu.reference(robot12, p, tu.SIM_DT, rows, before, mask, info, stats)
    bad = tu.same(got, want)
    assert bad == [], (bad, [names[i] for i in np.nonzero(got.fired != want.fired)[0]])
    assert np.array_equal(rows_after.view(np.uint64), rows.view(np.uint64))                      # the rows are read only
    return before, got


@pytest.mark.parametrize("masked", (False, True), ids=("all", "masked"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("robot12", (True, False), ids=("solo12", "solo8"))
def test_kernel_equals_the_table_bitwise(gpu_device, robot12, n, masked):
    """Every crafted row of the host test: n = 130 holds them all in one launch (row i = case i mod their number), n = 6 walks them
    six at a time.  done, reward, fired_out, the info arrays, the ep_stats and term_stats columns equal the numpy table bit for bit;
    what the table leaves alone still holds its fill (0xAA bytes in fired_out of masked rows and in timeout / success / episode_reward
    of rows where nothing fired, the sums' previous values)."""
    p = tu.params(robot12)
    ncases = len(tu.cases(robot12))
    total = n if n >= ncases else -(-ncases // n) * n
    rows, done, reward, names = tu.batch(robot12, total)
    fired_any = 0
    for k in range(0, total, n):
        sl = slice(k, k + n)
        mask = ((np.arange(n) + k // n) % 3 != 1) if masked else None
        before, got = _check(robot12, p, rows[sl], done[sl], reward[sl], names[sl], mask, seed=k)
        live = np.ones(n, bool) if mask is None else mask
        assert np.all(got.fired[~live] == tu.POISON8) and np.all(got.fired[live] != tu.POISON8)
        quiet = ~live | (got.fired == 0)
        assert np.all(got.timeout[quiet] == tu.POISON8) and np.all(got.success[quiet] == tu.POISON8)
        assert np.all(got.ep_reward.view(np.uint32)[quiet] == tu.POISON32)
        assert np.array_equal(got.reward.view(np.uint32)[quiet], before.reward.view(np.uint32)[quiet])
        assert np.array_equal(got.ep_stats.view(np.uint32)[9], before.ep_stats.view(np.uint32)[9])       # the NaN-guard count is never touched
        fired_any += int((got.fired[live] != 0).sum())
    assert fired_any >= (20 if not masked else 10)
    if n == 130:                                        # the NULL blocks, a bool mask, a single rule, no min_steps
        sl = slice(0, n)
        _check(robot12, p, rows[sl], done[sl], reward[sl], names[sl], info=False)
        _check(robot12, p, rows[sl], done[sl], reward[sl], names[sl], stats=False, mask=np.arange(n) % 2 == 0)
        _check(robot12, p, rows[sl], done[sl], reward[sl], names[sl], info=False, stats=False)
        _check(robot12, p.but(rules=tu.CONTACT, min_steps=0, terminal_reward=-2.5), rows[sl], done[sl], reward[sl], names[sl])
        _check(robot12, p.but(rules=tu.JOINT | tu.HEIGHT, contact_force_min=0.0), rows[sl], done[sl], reward[sl], names[sl])


# ---- twin handles
#        name          robot         task        f64  H  environment
TWINS = {"walk12":      (ROBOT_SOLO12, TASK_WALK,  0, 1, {}),
         "walk12_lane": (ROBOT_SOLO12, TASK_WALK,  0, 1, {"SOLORL_TEAM": "0"}),
         "stand8":      (ROBOT_SOLO8,  TASK_STAND, 1, 0, {})}
TWIN_STEPS = {"walk12": 40, "walk12_lane": 40, "stand8": 40}
# state members that differ between the in-step auto-reset and solorl_reset_masked: none is known
TWIN_MEMBERS_LEFT_OUT = ()


def _twin_cfg(case, **fields):
    robot, task, f64, H, _ = TWINS[case]
    c = default_config(robot, task)
    c.num_history_stack = H
    if f64:
        c.precision = PRECISION_F64
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _make(case, N, monkeypatch, seed=5, off=3, **fields):
    from solorl_amd.vec_env import SoloVecEnv
    for k in ("SOLORL_SORT", "SOLORL_TEAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in TWINS[case][4].items():
        monkeypatch.setenv(k, v)                     # (read at solorl_create)
    return SoloVecEnv(_twin_cfg(case, **fields), N, device=DEV, seed=seed, env_id_offset=off)


def _actions(N, A, steps, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return [(torch.rand(N, A, device=DEV, generator=g) * 2 - 1).contiguous() for _ in range(steps)]


def _member_diff(a, b):
    """the members of solorl_env_state whose bytes differ between two StateBatches"""
    x, y = a.bytes(), b.bytes()
    out = []
    for name, ctype in EnvState._fields_:
        f = getattr(EnvState, name)
        if name not in TWIN_MEMBERS_LEFT_OUT and not torch.equal(x[:, f.offset:f.offset + f.size], y[:, f.offset:f.offset + f.size]):
            out.append(name)
    return out


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", tuple(TWINS))
def test_twin_run_equals_the_engines_own_fall_rule(gpu_device, monkeypatch, case, N):
    """A ends episodes itself (z < 0.05; the time limit of 400 is out of reach); B has disable_termination and the same rule through
    solorl_terminate and solorl_reset_masked, which promises the draw an in-step auto-reset would make next.  A float z is below
    0.05f exactly when it is below the double 0.05 (0.05f > 0.05 and no float lies between them).  After every step: observations,
    rewards, done flags, the info fields, ep_stats and the state rows, bit for bit."""
    A = _make(case, N, monkeypatch)
    B = _make(case, N, monkeypatch, disable_termination=1)
    B.set_termination(base_height=0.05, terminal_reward=-10, min_steps=0)
    assert torch.equal(A.reset(), B.reset())
    sa, sb = StateBatch(N, DEV), StateBatch(N, DEV)
    falls = 0
    for t, act in enumerate(_actions(N, A.act_dim, TWIN_STEPS[case])):
        oa, ra, da, ia = A.step_inplace(act)
        ob, rb, db, ib = B.step_inplace(act)
        assert not bool((da != 0)[ia["timeout"] != 0].any()), t                            # A ends by the fall rule alone
        assert torch.equal(da, db), (t, da.nonzero().view(-1).tolist(), db.nonzero().view(-1).tolist())
        assert torch.equal(B.last_termination, db), t                                      # bit 1 = HEIGHT, and nothing else ends B's episodes
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), t
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), (t, (oa != ob).any(dim=1).nonzero().view(-1).tolist())
        bad = [k for k in ia if not torch.equal(ia[k], ib[k])]
        assert bad == [], (t, bad)
        assert torch.equal(A._ep_stats.view(torch.int32), B._ep_stats.view(torch.int32)), t
        diff = _member_diff(A.get_states(out=sa), B.get_states(out=sb))
        assert diff == [], (t, diff)
        falls += int(da.sum())
    print("twin %s N=%d: %d episodes ended by the fall rule in %d steps" % (case, N, falls, TWIN_STEPS[case]))
    assert falls >= 3                                                                      # a run without falls proves nothing
    st = B.termination_stats()
    assert st["term/episodes"] == falls and st["term/early"] == 1.0 and st["term/height"] == 1.0
    A.close(); B.close()


# ---- 3: composition
WEIGHTS = {"lin_vel_z": -2.0, "action_rate": -0.01, "foot_slip": -0.1, "tracking_lin_vel": 1.0, "tracking_yaw_rate": 0.5}
GROUPS = {"height": 0.01, "orientation": 0.03, "lin_vel": 0.1, "ang_vel": 0.2, "joint_pos": 0.01, "joint_vel": 1.5}
WALK_CMD = dict(lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), yaw_rate=(-1.0, 1.0), interval=(20, 30), obs_scale=(2.0, 2.0, 0.25))
RULES = dict(contacts=["base"], max_tilt_deg=60, min_steps=1, terminal_reward=-7.5)


def _composed(N, noise):
    from solorl_amd.vec_env import SoloVecEnv
    c = default_config(ROBOT_SOLO12, TASK_WALK)
    c.num_history_stack = 1
    env = SoloVecEnv(c, N, device=DEV, seed=5, env_id_offset=3, commands=WALK_CMD)
    env.set_reward_shaping(WEIGHTS)
    env.set_actuation(delay=(0, 2), gain_range=0.2)
    if noise:
        env.set_obs_noise(GROUPS)
    env.set_termination(**RULES)
    return env


def _params_of(p):
    return tu.Params(p.rules, p.min_steps, p.contact_prims, p.min_height, p.min_up_z, p.contact_force_min, list(p.joint_lo), list(p.joint_hi), p.terminal_reward)


@pytest.mark.parametrize("N", SIZES)
def test_composition_with_shaping_actuation_commands_and_noise(gpu_device, N):
    """A has everything set; C is A without the noise, so its observation rows are the clean ones (noise changes nothing but them: the
    actions are given).  For every env a rule ends: the reward is the terminal reward, the shaping episode count rises by one, the
    actuator draws a new episode at the next call, the command is drawn anew, the observation row is the reset observation plus this
    call's noise; last_termination and termination_stats() equal a recount (tests/term_util.py) from the rows taken before the reset.
    min_steps = 1: a row the engine itself ended holds timestep 0 and is recounted as not fired, as the call treats it."""
    from solorl_amd.channel import obs_noise
    A, C_ = _composed(N, True), _composed(N, False)
    D = A.engine_obs_dim
    A.reset(); C_.reset()
    p = _params_of(A._term)
    ended, by_rule, episodes = 0, np.zeros(4, dtype=np.int64), 0
    pending = None                                       # the envs ended by the last step and their actuator episode counts
    for t, act in enumerate(_actions(N, 12, 40 if N == 6 else 24)):
        count = A._noise_count.clone()
        ep0, draws0 = A._shape_ep[0].clone(), A._cmd_mem.draws.clone()
        oa, ra, da, ia = A.step_inplace(act)
        oc, rc, dc, _ = C_.step_inplace(act)
        if pending is not None:                          # the actuator row restarted with the action that followed
            idx, before = pending
            assert torch.equal(A._act_mem.episodes[idx], before[idx] + 1) and bool((A._act_mem.fill[idx] <= 1).all()), t
        rows = A._term_states.data.cpu().numpy()         # the get_states rows of this step, taken before the reset
        recount = np.array([tu.fired_bits(True, p, A.cfg.sim_dt, r) for r in rows], dtype=np.uint8)
        fired = A.last_termination.cpu().numpy()
        assert np.array_equal(fired, recount), (t, np.nonzero(fired != recount)[0].tolist())
        assert torch.equal(da, dc) and torch.equal(ra.view(torch.int32), rc.view(torch.int32)) and torch.equal(A.last_termination, C_.last_termination), t
        idx = torch.from_numpy(np.nonzero(fired)[0]).to(DEV)
        assert bool((da[idx] == 1).all()) and bool((ra[idx] == -7.5).all()), t
        assert bool((ia["timeout"][idx] == 0).all()) and bool((ia["episode_reward"][idx] == -7.5).all()), t
        assert torch.equal(A._shape_ep[0][idx], ep0[idx] + 1) and bool((A.last_shaping_terms[idx] == 0).all()), t
        assert bool((A._act_restart[idx] == 1).all()), t
        assert torch.equal(A._cmd_mem.draws[idx], draws0[idx] + 1), t
        # the observation rows: C's are the reset observation (its engine's current one), A's are those plus this call's noise
        clean = C_.get_observation()
        assert torch.equal(oc[idx].view(torch.int32), clean[idx].view(torch.int32)), t
        noisy = obs_noise(A._seed, A._id0, A._noise_scale, count, oc[:, :D].contiguous())
        assert torch.equal(oa[:, :D].view(torch.int32), noisy.view(torch.int32)) and torch.equal(oa[:, D:], oc[:, D:]), t
        if len(idx):
            assert not torch.equal(oa[idx][:, :D], oc[idx][:, :D])
            ts = A.get_states().timestep
            assert bool((ts[idx] == 0).all()), t         # they stand in a new episode
        pending = (idx, A._act_mem.episodes.clone()) if len(idx) else None
        ended += len(idx)
        episodes += int(da.sum())
        for k in range(4):
            by_rule[k] += int(((fired >> k) & 1).sum())
    print("composition N=%d: %d of %d finished episodes ended by a rule (tilt %d, contact %d)" % (N, ended, episodes, by_rule[1], by_rule[2]))
    assert ended >= 3 and by_rule[0] == 0 and by_rule[3] == 0                             # a run in which no rule fires proves nothing
    if N == 130:
        assert by_rule[1] >= 1 and by_rule[2] >= 1                                        # both rules ended episodes
    st = A.termination_stats()
    assert st["term/episodes"] == episodes and set(st) == {"term/episodes", "term/early", "term/tilt", "term/contact"}
    assert st["term/early"] == ended / episodes and st["term/tilt"] == by_rule[1] / episodes and st["term/contact"] == by_rule[2] / episodes
    assert A.termination_stats()["term/episodes"] == 0                                    # the call started a new window
    A.close(); C_.close()


# ---- 4: capture
def test_three_captured_steps_equal_an_eager_twin(gpu_device):
    N = 130
    A, B = _composed(N, True), _composed(N, True)
    A.reset(); B.reset()
    acts = _actions(N, 12, 12 + 12, seed=21)
    for a in acts[:12]:                                  # both fall about for a while: the rules fire from here on
        A.step_inplace(a); B.step_inplace(a)
    act = [torch.zeros(N, 12, device=DEV) for _ in range(3)]
    out = [(torch.zeros(N, A.obs_dim, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)) for _ in range(3)]
    fired = [torch.zeros(N, dtype=torch.uint8, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(3):
            A.step_inplace(act[k], obs_out=out[k][0], rew_out=out[k][1], done_out=out[k][2])
            fired[k].copy_(A.last_termination)
    seen = 0
    for r in range(4):
        for k in range(3):
            act[k].copy_(acts[12 + 3 * r + k])
        graph.replay()
        for k in range(3):
            ob, rb, db, _ = B.step_inplace(acts[12 + 3 * r + k])
            torch.cuda.synchronize()
            assert torch.equal(out[k][0].view(torch.int32), ob.view(torch.int32)) and torch.equal(out[k][1].view(torch.int32), rb.view(torch.int32)), (r, k)
            assert torch.equal(out[k][2], db) and torch.equal(fired[k], B.last_termination), (r, k)
            seen += int((fired[k] != 0).sum())
        assert torch.equal(A._term_stats, B._term_stats) and torch.equal(A._ep_stats.view(torch.int32), B._ep_stats.view(torch.int32)), r
        assert torch.equal(A._shape_mem.data.view(torch.int64), B._shape_mem.data.view(torch.int64)) and torch.equal(A._cmd_mem.data.view(torch.int64), B._cmd_mem.data.view(torch.int64)), r
        assert torch.equal(A.get_states().bytes(), B.get_states().bytes()), r
    assert seen >= 3                                     # rules fired inside the replayed steps
    A.close(); B.close()


# ---- 5 and 6
def test_refused_paths_and_off_is_off(gpu_device, monkeypatch):
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import Box, make_vec_envs
    N = 8
    torch.manual_seed(3)
    P = policy_params(Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(DEV))
    plain, env = _make("walk12", N, monkeypatch), _make("walk12", N, monkeypatch)
    names = ("_term", "_term_states", "_term_stats", "_term_eps", "last_termination")
    assert all(getattr(plain, k) is None for k in names)                                  # off: nothing is allocated
    with pytest.raises(_native.SoloRLError, match="termination_stats"):
        plain.termination_stats()
    assert plain.step_act_supported(P) and plain.rollout_supported(P)
    env.set_termination(dict(base_height=0.12), max_tilt_deg=45)
    assert env._term.rules == 3 and env.last_termination.dtype == torch.uint8 and tuple(env._term_stats.shape) == (5, N)
    assert not env.step_act_supported(P) and not env.rollout_supported(P)
    plain.reset(); env.reset()
    acts = torch.zeros(2, N, 12, device=DEV)
    val, lp = torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV)
    with pytest.raises(_native.SoloRLError, match="step_n.*termination"):
        env.step_n_inplace(acts)
    with pytest.raises(_native.SoloRLError, match="step_n.*termination"):
        env.step_n(acts)
    with pytest.raises(_native.SoloRLError, match="rollout_inplace.*termination"):
        env.rollout_inplace(acts, P, None, val, lp)
    with pytest.raises(_native.SoloRLError, match="step_act_inplace.*termination"):
        env.step_act_inplace(acts[0], P, None, val[0], acts[1], lp[0])
    with pytest.raises(ValueError, match="max_tilt"):
        env.set_termination(max_tilt=45)
    assert env._term.rules == 3                                                           # a refused call leaves it as it was
    env.set_termination(None)
    assert all(getattr(env, k) is None for k in names)
    assert env.step_act_supported(P) and env.rollout_supported(P)
    # off is off: the env that set and cleared it steps like the one that never had it, through every path
    g = torch.Generator(device=DEV); g.manual_seed(4)
    rnd = lambda *s: (torch.rand(*s, device=DEV, generator=g) * 2 - 1).contiguous()
    for t in range(12):
        a = rnd(N, 12)
        (o1, r1, d1, i1), (o2, r2, d2, i2) = plain.step_inplace(a), env.step_inplace(a)
        assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(r1, r2) and torch.equal(d1, d2), t
    a2, v1, v2, l1, l2 = rnd(2, N, 12), torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV)
    (o1, r1, d1, _), (o2, r2, d2, _) = plain.step_n_inplace(a2), env.step_n_inplace(a2)
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    n1, n2 = a2.clone(), a2.clone()
    plain.step_act_inplace(a2[0], P, None, v1[0], n1[1], l1[0]); env.step_act_inplace(a2[0], P, None, v2[0], n2[1], l2[0])
    assert torch.equal(n1, n2) and torch.equal(v1, v2) and torch.equal(l1, l2)
    plain.rollout_inplace(n1, P, None, v1, l1); env.rollout_inplace(n2, P, None, v2, l2)
    assert torch.equal(n1, n2) and torch.equal(v1, v2)
    assert torch.equal(plain.get_states().bytes(), env.get_states().bytes())
    plain.close(); env.close()
    config = dict(episode_length=10, solo12=True, task="walk", num_history_stack=1)
    made = make_vec_envs(config, N, device=DEV, termination=dict(contacts=["base", "shoulders"], max_tilt_deg=60, min_steps=2))
    assert made._term.rules == 6 and made._term.min_steps == 2
    with pytest.raises(ValueError, match="base_hight"):
        make_vec_envs(config, N, device=DEV, termination=dict(base_hight=0.1))
    made.close()


# ---- training with the flag
def test_training_with_a_termination_takes_the_two_launch_rollout(gpu_device, monkeypatch):
    """train() for three updates of 64 walk12 envs x 16 steps with --termination under HIP graphs: GraphedRollout gives up the policy
    tail by itself, the rules fire, and the log carries their shares"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd import vec_env
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo import train as tr
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", "64", "--num-steps", "16",
            "--num-env-steps", str(64 * 16 * 3), "--mini-batch-size", "512", "--ppo-epoch", "2", "--use-gae", "--seed", "7", "--log-interval", "1",
            "--termination", os.path.join(ROOT, "configs", "termination_walk12.yaml")]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    args.termination = train_ppo.load_termination(args.termination, config)
    seen = {}

    def keep(name, f):
        def g(*a, **k):
            seen[name] = f(*a, **k)
            return seen[name]
        return g
    monkeypatch.setattr(vec_env, "make_vec_envs", keep("env", vec_env.make_vec_envs))
    monkeypatch.setattr(tr, "GraphedRollout", keep("graphed", tr.GraphedRollout))
    pol, hist = tr.train(args, config)
    torch.cuda.synchronize()
    assert len(hist) == 3 and all(torch.isfinite(q).all() for q in pol.parameters())
    env, graphed = seen["env"], seen["graphed"]
    assert env._term is not None and not graphed.step_act and graphed.windows is None and graphed.graph is not None
    for rec in hist:
        assert {"term/episodes", "term/early", "term/tilt", "term/contact"} <= set(rec)
    assert sum(rec["term/episodes"] for rec in hist) == sum(rec["episodes"] for rec in hist) > 0
    assert any(rec["term/early"] > 0 for rec in hist if rec["term/episodes"])
    env.close()


def test_eval_ppo_with_a_termination(gpu_device, tmp_path, capsys):
    """eval_ppo.py --termination: the summary carries the share of the finished episodes each rule ended (an untrained, stochastic
    policy: it falls within a few dozen steps)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval_ppo
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(5)
    pol = Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64})
    torch.save({"update": 0, "state_dict": pol.state_dict(), "ob_rms": None}, os.path.join(str(tmp_path), "solo.pt"))
    r = eval_ppo.main(["--checkpoint-dir", str(tmp_path), "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk",
                       "--num-agents", "16", "--num-runs", "4", "--max-steps", "120",
                       "--termination", os.path.join(ROOT, "configs", "termination_walk12.yaml")])
    out = capsys.readouterr().out
    ts = r["termination"]
    assert "early termination over %d finished episodes" % ts["term/episodes"] in out and "contact" in out and "tilt" in out
    assert set(ts) == {"term/episodes", "term/early", "term/tilt", "term/contact"} and ts["term/episodes"] >= r["episodes"] >= 4
    assert 0.0 < ts["term/early"] <= 1.0 and ts["term/early"] <= ts["term/tilt"] + ts["term/contact"]
