"""solorl_shape_reward on the GPU (include/solorl.h; solorl_amd/shaping.py, SoloVecEnv.set_reward_shaping).

1. The kernel's outputs against the stand-alone host program's (tests/host/shape_main.cpp: the same per-env function compiled by g++)
   to |err| <= 1e-10 max(1, |value|), integers exactly, the reward to one f32 ulp -- both robots, n = 1, 5, one more than the kernel's
   envs per workgroup, and two workgroups + 3 (a ragged last one); every optional pointer NULL once.
2. Masked rows keep every byte (a whole workgroup among them), done rows follow the rule bit for bit.
3. Twin handles, one with shaping: the physics is bitwise the same, the shaped reward is the unshaped one plus the weighted terms,
   the terminal reward is untouched, shaping_stats() equals the test's own running sums.
4. A captured step_inplace with shaping replays to what eager steps of a twin give, bit for bit.
5. step_act_inplace with shaping pays what step_inplace does, and the return normaliser receives the shaped reward.
6. The K-step calls are refused while shaping is set, and nothing is allocated while it never was.
7. The torques and power terms are sums over the recorded torques on an env that records them, 0 on one that does not."""
import numpy as np
import pytest
import torch

from solorl_amd import _native
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from solorl_amd.shaping import ENVS_PER_WORKGROUP, EP_FIELDS, SHAPE_TERMS, TERMS, ShapeMem, shape_reward
from solorl_amd.state import StateBatch
from tests import shape_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 5, ENVS_PER_WORKGROUP + 1, 2 * ENVS_PER_WORKGROUP + 3)
WEIGHTS = {"lin_vel_z": -2.0, "ang_vel_xy": -0.05, "orientation": -1.0, "base_height": -10.0, "joint_vel": -1e-3, "joint_acc": -2.5e-7,
           "action_rate": -0.01, "foot_slip": -0.1, "foot_clearance": -1.0, "foot_force": -0.01, "feet_air_time": 1.0, "collision": -1.0,
           "tracking_lin_vel": 1.0, "tracking_yaw_rate": 0.5}
PARAMS = dict(foot_force_max=15.0, air_time_target=0.1)


def _dev(a):
    return torch.tensor(np.array(a), device=DEV)


def _device_call(c, flags=su.F_ALL, mask=None):
    """one solorl_shape_reward launch on case c -> (mem, reward, terms, ep) as numpy, as tests/shape_util.run_shape_main gives them"""
    sb, mem = StateBatch(data=_dev(c.states)), ShapeMem(data=_dev(c.mem))
    reward, terms, ep = _dev(c.reward), _dev(c.terms), _dev(c.ep)
    shape_reward(c.cfg, c.params, sb, _dev(c.actions), _dev(c.done) if flags & su.F_DONE else None, mem, reward if flags & su.F_REWARD else None,
                 terms_out=terms if flags & su.F_TERMS else None, ep_out=ep if flags & su.F_EP else None, mask=None if mask is None else _dev(mask))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (mem.data, reward, terms, ep))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("robot", (0, 1))
def test_kernel_rows_equal_the_host_program(robot, n):
    c = su.case(robot, n)
    su.check_outputs(c, _device_call(c), su.run_shape_main(c))


@pytest.mark.parametrize("absent", (su.F_DONE, su.F_REWARD, su.F_TERMS, su.F_EP))
def test_every_optional_pointer_null_once(absent):
    c = su.case(1, SIZES[2])
    flags = su.F_ALL & ~absent
    su.check_outputs(c, _device_call(c, flags=flags), su.run_shape_main(c, flags=flags), flags=flags)


@pytest.mark.parametrize("robot", (0, 1))
def test_masked_rows_keep_every_byte_and_done_rows_follow_the_rule(robot):
    c = su.case(robot, SIZES[3])
    mask = (np.arange(c.n) % 3 != 1).astype(np.uint8) * 7
    mask[ENVS_PER_WORKGROUP:2 * ENVS_PER_WORKGROUP] = 0                  # a workgroup with nothing to do
    off = mask == 0
    assert (c.done[~off] != 0).any() and (c.done[~off] == 0).any()
    for poison64, poison32 in ((np.float64("nan"), np.float32("nan")), (np.frombuffer(b"\xa5" * 8, np.float64)[0], np.frombuffer(b"\xa5" * 4, np.float32)[0])):
        p = su.types.SimpleNamespace(**vars(c))
        p.states, p.mem, p.terms, p.ep, p.reward, p.actions = (a.copy() for a in (c.states, c.mem, c.terms, c.ep, c.reward, c.actions))
        p.states[off] = poison64; p.mem[off] = poison64; p.terms[off] = poison64; p.ep[:, off] = poison64
        p.reward[off] = poison32; p.actions[off] = poison32
        got = _device_call(p, mask=mask)
        su.check_outputs(p, got, su.run_shape_main(p, mask=mask), mask=mask)       # (masked and done rows: bit for bit)
        for g, was in zip(got, (p.mem, p.reward, p.terms)):
            assert (su.bits(g).reshape(c.n, -1)[off] == su.bits(was).reshape(c.n, -1)[off]).all()
        assert (su.bits(got[3]).reshape(EP_FIELDS, c.n, 8)[:, off] == su.bits(p.ep).reshape(EP_FIELDS, c.n, 8)[:, off]).all()


def _walk_cfg(episode_length=12, history=0):
    c = default_config(ROBOT_SOLO12, TASK_WALK)
    c.episode_length, c.num_history_stack = episode_length, history
    return c


def _actions(T, N, seed=1234):
    g = torch.Generator(); g.manual_seed(seed)                # (on the CPU: the same rows whatever the device)
    return (torch.rand(T, N, 12, generator=g) * 3 - 1.5).to(DEV)


def _one_ulp(got, ref):
    return bool((torch.abs(got.double() - ref.double()) <= torch.abs(torch.nextafter(ref, torch.full_like(ref, float("inf"))) - ref).double()).all())


def test_twin_handles_shaping_changes_the_reward_and_nothing_else(gpu_device):
    """Two handles, the same seed and actions, one with shaping, 40 steps with episodes of 12 (an oracle rollout of these actions has 24
    finished episodes and 32 first contacts of a foot: the test fails if the engine's run has none)."""
    from solorl_amd.vec_env import SoloVecEnv
    N, T = 8, 40
    plain, shaped = (SoloVecEnv(_walk_cfg(), N, device=DEV, seed=11) for _ in range(2))
    assert shaped.last_shaping_terms is None
    shaped.set_reward_shaping(WEIGHTS, **PARAMS)
    w = torch.tensor(list(shaped._shape_params.weight), dtype=torch.float64, device=DEV)
    assert torch.equal(plain.reset(), shaped.reset())
    A = _actions(T, N)
    ep_sum = torch.zeros(N, SHAPE_TERMS, dtype=torch.float64, device=DEV)
    total, count, firsts = torch.zeros(SHAPE_TERMS, dtype=torch.float64, device=DEV), 0, 0
    for t in range(T):
        o1, r1, d1, i1 = plain.step(A[t])
        o2, r2, d2, i2 = shaped.step(A[t])
        assert torch.equal(o1, o2) and torch.equal(d1, d2), t                     # shaping changes no physics
        for k in i1.tensors:
            assert torch.equal(i1.tensors[k], i2.tensors[k]), (t, k)
        terms, dn = shaped.last_shaping_terms, d1.bool()
        s = torch.zeros(N, dtype=torch.float64, device=DEV)
        for k in range(SHAPE_TERMS):                                              # fp64, index order
            s = s + w[k] * terms[:, k]
        want = (r1.view(-1).double() + s).float()
        assert _one_ulp(r2.view(-1)[~dn], want[~dn]), t
        assert torch.equal(r2.view(-1)[dn], r1.view(-1)[dn]) and not terms[dn].any(), t       # the terminal reward is the engine's
        assert torch.isfinite(terms).all()
        firsts += int((terms[~dn, TERMS.index("feet_air_time")] != 0).sum())
        ep_sum[~dn] += (w * terms)[~dn]
        total += ep_sum[dn].sum(0); count += int(dn.sum())
        ep_sum[dn] = 0.0
    assert count > 0 and firsts > 0, (count, firsts)
    assert (shaped._shape_mem.valid == (~dn).int()).all()
    st = shaped.shaping_stats()
    assert st["episodes"] == count
    for k, name in enumerate(TERMS):
        ref = float(total[k]) / count
        assert abs(st["sr/" + name] - ref) <= 1e-10 * max(1.0, abs(ref)), (name, st["sr/" + name], ref)
    assert shaped.shaping_stats()["episodes"] == 0                                # reset=True zeroed the sums
    # reset() and reset_masked() clear the memory of the envs they reset
    mask = torch.zeros(N, dtype=torch.bool, device=DEV); mask[::3] = True
    before = shaped._shape_mem.data.clone()
    shaped.reset_masked(mask)
    assert not shaped._shape_mem.data[mask].any() and torch.equal(shaped._shape_mem.data[~mask], before[~mask])
    shaped.reset()
    assert not shaped._shape_mem.data.any()
    plain.close(); shaped.close()


def test_captured_step_with_shaping_replays_like_eager_steps(gpu_device):
    from solorl_amd.vec_env import SoloVecEnv
    N = 8
    eager, graphed = (SoloVecEnv(_walk_cfg(episode_length=4), N, device=DEV, seed=7) for _ in range(2))
    for e in (eager, graphed):
        e.set_reward_shaping(WEIGHTS, **PARAMS)
        e.reset()
    A = _actions(6, N, seed=99)
    a = A[0].clone()
    r0 = eager.step_inplace(a)[1].clone()
    assert torch.equal(graphed.step_inplace(a)[1], r0)            # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = graphed.step_inplace(a)
    dones = 0
    for t in range(1, 6):
        a.copy_(A[t])
        g.replay()
        o, r, d, _ = eager.step_inplace(A[t].contiguous())
        assert torch.equal(out[0], o) and torch.equal(out[1], r) and torch.equal(out[2], d), t
        assert torch.equal(graphed.last_shaping_terms, eager.last_shaping_terms), t
        dones += int(d.sum())
    assert dones > 0
    assert torch.equal(graphed._shape_mem.bytes(), eager._shape_mem.bytes()) and torch.equal(graphed._shape_ep, eager._shape_ep)
    assert float(eager._shape_ep[0].sum()) >= dones              # every finished episode was counted
    eager.close(); graphed.close()


def _policy(O, A, seed=3):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}).to(DEV)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
    return pol


def test_step_act_inplace_with_shaping_and_return_normalisation(gpu_device):
    """step_act_inplace pays what step_inplace pays on a twin driven by the same actions (which a separate policy act on the twin's
    observations reproduces), and with norm_ret the normaliser's input is the shaped reward: a twin normaliser fed the twin's shaped
    rewards gives the same rewards and statistics, bit for bit."""
    from solorl_amd.normalize import VecNormalizer
    from solorl_amd.ppo.fused import policy_act, policy_params
    from solorl_amd.vec_env import SoloVecEnv
    N, K = 8, 14
    cfg = _walk_cfg(episode_length=6, history=1)
    P = policy_params(_policy(76, 12))
    fused = SoloVecEnv(cfg, N, device=DEV, seed=5, norm_ret=True, gamma=0.97)
    twin = SoloVecEnv(cfg, N, device=DEV, seed=5)
    plain = SoloVecEnv(cfg, N, device=DEV, seed=5)
    norm = VecNormalizer(N, 76, torch.device(DEV), False, True, 10.0, 10.0, 0.97, 1e-8)
    for e in (fused, twin):
        e.set_reward_shaping(WEIGHTS, **PARAMS)
    assert fused.step_act_supported(P) and not fused.rollout_supported(P)
    o0 = fused.reset()
    assert torch.equal(o0, twin.reset()) and torch.equal(o0, plain.reset())
    g = torch.Generator(device=DEV); g.manual_seed(13)
    noise = torch.randn(K + 1, N, 12, device=DEV, generator=g)
    act = torch.zeros(K + 1, N, 12, device=DEV); act[0] = torch.rand(N, 12, device=DEV, generator=g) * 2 - 1
    val, lp = torch.zeros(K + 1, N, device=DEV), torch.zeros(K + 1, N, device=DEV)
    differs = False
    for k in range(K):
        o, r, d, _ = fused.step_act_inplace(act[k], P, noise[k + 1].contiguous(), val[k + 1], act[k + 1], lp[k + 1])
        o2, r2, d2, _ = twin.step_inplace(act[k].contiguous())
        assert torch.equal(o, o2) and torch.equal(d, d2), k
        v2, a2, l2 = torch.zeros(N, 1, device=DEV), torch.zeros(N, 12, device=DEV), torch.zeros(N, 1, device=DEV)
        policy_act(P, o2, noise[k + 1].contiguous(), v2, a2, l2)
        assert torch.allclose(a2, act[k + 1], atol=1e-4, rtol=1e-4), k
        differs = differs or not torch.equal(r2, plain.step_inplace(act[k].contiguous())[1])
        want = norm.rewards(r2.clone(), d2, 1, True)
        assert torch.equal(r, want), k
        assert torch.equal(fused._norm.ret_stats, norm.ret_stats) and torch.equal(fused._norm.ret, norm.ret), k
        assert torch.equal(fused.last_shaping_terms, twin.last_shaping_terms), k
    assert differs                                               # the shaped reward is not the plain one
    assert torch.equal(fused._shape_mem.bytes(), twin._shape_mem.bytes()) and float(fused._shape_ep[0].sum()) > 0
    for e in (fused, twin, plain):
        e.close()


def test_torque_terms_read_the_recorded_torques(gpu_device):
    """solorl_get_states leaves the rows' tau 0: on an env that records the applied torques the torques and power terms are sums over
    them (fp64 sums of 12 products: 1e-12 relative), on one that does not they are 0."""
    from solorl_amd.vec_env import SoloVecEnv
    N = 8
    rec, bare = SoloVecEnv(_walk_cfg(), N, device=DEV, seed=3, applied_torque=True), SoloVecEnv(_walk_cfg(), N, device=DEV, seed=3)
    A = _actions(3, N, seed=5)
    for e in (rec, bare):
        e.set_reward_shaping({"torques": -1e-4, "power": -1e-3})
        e.reset()
        for t in range(3):
            o, r, d, _ = e.step_inplace(A[t].contiguous())
    live = d == 0
    tau, qd, terms = rec.record_applied_torque().double(), rec._shape_states.qd, rec.last_shaping_terms
    k_tq, k_pw = TERMS.index("torques"), TERMS.index("power")
    assert live.any() and (tau[live] != 0).any()
    assert torch.allclose(terms[live, k_tq], (tau ** 2).sum(1)[live], rtol=1e-12, atol=0.0)
    assert torch.allclose(terms[live, k_pw], (tau * qd).abs().sum(1)[live], rtol=1e-12, atol=0.0)
    assert (terms[live, k_tq] > 0).all() and not bare.last_shaping_terms[:, [k_tq, k_pw]].any()
    rec.close(); bare.close()


def test_k_step_calls_are_refused_and_the_off_state_allocates_nothing(gpu_device):
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import SoloVecEnv
    N = 8
    env = SoloVecEnv(_walk_cfg(history=1), N, device=DEV, seed=3)
    P = policy_params(_policy(76, 12))
    for name in ("_shape_params", "_shape_mem", "_shape_states", "_shape_ep", "last_shaping_terms"):
        assert getattr(env, name) is None, name
    env.reset()
    z = torch.zeros(2, N, 12, device=DEV)
    v = torch.zeros(2, N, device=DEV)
    env.step_n(z); env.step_n_inplace(z); env.rollout_inplace(z.clone(), P, None, v, v.clone())
    assert env.rollout_supported(P)
    for name in ("_shape_params", "_shape_mem", "_shape_states", "_shape_ep", "last_shaping_terms"):
        assert getattr(env, name) is None, name                  # stepping without shaping allocates none of it
    with pytest.raises(ValueError, match="foot_slop"):
        env.set_reward_shaping({"foot_slop": 1.0})
    env.set_reward_shaping({"foot_slip": -0.1})
    assert not env.rollout_supported(P) and env.last_shaping_terms.shape == (N, SHAPE_TERMS) and env._shape_ep.shape == (EP_FIELDS, N)
    for call in (lambda: env.step_n(z), lambda: env.step_n_inplace(z), lambda: env.rollout_inplace(z.clone(), P, None, v, v.clone())):
        with pytest.raises(_native.SoloRLError, match="reward shaping"):
            call()
    env.step_inplace(z[0])
    assert env.last_shaping_terms.any()
    env.set_reward_shaping(None)
    assert env.last_shaping_terms is None and env._shape_mem is None and env.rollout_supported(P)
    env.step_n(z); env.step_n_inplace(z); env.rollout_inplace(z.clone(), P, None, v, v.clone())
    torch.cuda.synchronize()
    env.close()
