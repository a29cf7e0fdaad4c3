"""Time-limit bootstrapping on the GPU (include/solorl.h solorl_compute_returns_tl; SoloVecEnv.step_inplace(timeout_out=) and its kin;
RolloutStorage(bootstrap_timeouts=True); GraphedRollout): the kernel against the storage's CPU formulation and, bit for bit, against
solorl_compute_returns where no timeout occurs; the engine's timeout flags in caller-owned rows through every step call; and a
captured rollout against the eager one."""
import numpy as np
import pytest
import torch

from tests import timelimit_util as tu

pytestmark = pytest.mark.gpu

T_ENV, EP_LEN = 12, 5


# ---- the kernel
# (9, 257): past the walk's unroll of 8, and one env past the launch's 256-thread block
@pytest.mark.parametrize("use_gae", [True, False])
@pytest.mark.parametrize("T,N", [(1, 1), (9, 257), (16, 64)])
def test_kernel_matches_the_cpu_storage_path(gpu_device, T, N, use_gae):
    """same case construction and bound (allclose, atol 1e-5) as tests/test_timelimit_cpu.py holds the CPU path to against the fp64 loop"""
    c = tu.make_case(T, N, seed=T)
    g, h = tu.storage_of(c, gpu_device), tu.storage_of(c, torch.device("cpu"))
    g.compute_returns(tu.next_value_of(c, gpu_device), use_gae, tu.GAMMA, tu.LAM)
    h.compute_returns(tu.next_value_of(c, h.device), use_gae, tu.GAMMA, tu.LAM)
    rows = slice(0, T) if use_gae else slice(0, T + 1)
    print("(%d, %d) use_gae=%s: max |kernel - CPU path| = %.3g" % (T, N, use_gae, float((g.returns[rows].cpu() - h.returns[rows]).abs().max())))
    assert torch.allclose(g.returns[rows].cpu(), h.returns[rows], atol=1e-5)
    assert torch.equal(g.value_preds.cpu(), h.value_preds)
    ref, _ = tu.reference_returns(c, use_gae)
    assert torch.allclose(g.returns[rows, :, 0].cpu(), torch.from_numpy(ref[rows]).float(), atol=1e-5)


@pytest.mark.parametrize("use_gae", [True, False])
@pytest.mark.parametrize("flags", ["zero", "where_m_is_1"])
def test_kernel_writes_the_plain_kernels_bits_without_a_timeout(gpu_device, flags, use_gae):
    T, N = 9, 257
    c = tu.make_case(T, N, seed=2)
    c["timeouts"] = np.zeros_like(c["timeouts"]) if flags == "zero" else (c["timeouts"] * (c["masks"][1:] == 1)).astype(np.uint8)
    assert flags == "zero" or c["timeouts"].sum() > T * N // 4
    a, b = tu.storage_of(c, gpu_device), tu.storage_of(c, gpu_device, bootstrap=False)
    for s in (a, b):
        s.returns.fill_(7.0)
        s.compute_returns(tu.next_value_of(c, gpu_device), use_gae, tu.GAMMA, tu.LAM)
    assert torch.equal(a.returns, b.returns) and torch.equal(a.value_preds, b.value_preds)
    assert not bool((a.returns[:T] == 7.0).any())


def test_no_later_return_crosses_a_truncation_without_gae(gpu_device):
    """the kernel's select drops the carry at a truncated step, and so does the CPU path (tests/test_timelimit_cpu.py): a return that is
    not finite after the truncation leaves the returns before it finite, the same on both"""
    T, N = 9, 5
    c = tu.make_case(T, N, seed=4)
    c["masks"][:] = 1
    c["masks"][5], c["timeouts"][4] = 0, 1
    c["rewards"][6] = np.inf
    g, h = tu.storage_of(c, gpu_device), tu.storage_of(c, torch.device("cpu"))
    g.compute_returns(tu.next_value_of(c, gpu_device), False, tu.GAMMA, tu.LAM)
    h.compute_returns(tu.next_value_of(c, h.device), False, tu.GAMMA, tu.LAM)
    assert bool(torch.isfinite(g.returns[:5]).all()) and not bool(torch.isfinite(g.returns[5:7]).any())
    assert torch.allclose(g.returns.cpu(), h.returns, atol=1e-5)          # (equal infinities count as close)


# ---- the engine's flags in caller-owned rows
def _env(seed=3, n=8):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.vec_env import SoloVecEnv
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack, cfg.episode_length = 1, EP_LEN
    env = SoloVecEnv(cfg, n, device="cuda:0", seed=seed)
    return env, env.reset()


def _actions(n, dev):
    g = torch.Generator(device=dev); g.manual_seed(5)
    return torch.rand(T_ENV, n, 12, device=dev, generator=g) * 2 - 1


def test_step_calls_write_the_timeout_flags_into_caller_rows(gpu_device):
    """Solo12 walk, 8 envs, episode_length 5, 12 steps of random actions.  An equally seeded env stepped without ``timeout_out`` says
    what info["timeout"] is; the rows were filled with 0xAA first, so a flag that reads 0 or 1 was written by the step."""
    from solorl_amd.ppo.fused import policy_params
    n, dev = 8, gpu_device
    act = _actions(n, dev)
    ref_env, _ = _env()
    want, done = torch.empty(T_ENV, n, dtype=torch.uint8, device=dev), torch.empty(T_ENV, n, dtype=torch.uint8, device=dev)
    for t in range(T_ENV):
        _, _, d, info = ref_env.step_inplace(act[t])
        want[t], done[t] = info["timeout"], d
    ref_env.close()
    # the episode clock: five steps after the last end the time limit ends the episode -- steps 5 and 10 of an env that never fell
    clock = torch.zeros(n, dtype=torch.long, device=dev)
    for t in range(T_ENV):
        clock += 1
        due = clock == EP_LEN
        assert bool((done[t][due] == 1).all()) and bool((want[t][due] == 1).all()), t
        assert bool((want[t][(done[t] != 0) & ~due] == 0).all()), t
        clock[done[t] != 0] = 0
    assert int(want[EP_LEN - 1].sum()) > 0 and int(want[2 * EP_LEN - 1].sum()) > 0

    def check(rows, d_rows, name):
        assert torch.equal(d_rows, done), name
        assert bool(((rows == 0) | (rows == 1)).all()), name              # every byte was written
        assert torch.equal(rows[done != 0], want[done != 0]), name

    env, _ = _env()
    rows, d_rows = torch.full((T_ENV, n), 0xAA, dtype=torch.uint8, device=dev), torch.empty(T_ENV, n, dtype=torch.uint8, device=dev)
    for t in range(T_ENV):
        _, _, _, info = env.step_inplace(act[t], done_out=d_rows[t], timeout_out=rows[t])
        assert info["timeout"].data_ptr() == rows[t].data_ptr()           # the returned info holds the caller's row
    check(rows, d_rows, "step_inplace")
    assert len(env._info_alt) == T_ENV                                     # one info block per destination, kept
    env.close()

    env, _ = _env()
    pol = _path_independent_policy(dev)                                   # (any policy: its actions are not used)
    P = policy_params(pol)
    if env.step_act_supported(P):
        rows = torch.full((T_ENV, n, 1), 0xAA, dtype=torch.uint8, device=dev)       # [N, 1], as a storage's rows
        v, a, l = torch.empty(n, 1, device=dev), torch.empty(n, 12, device=dev), torch.empty(n, 1, device=dev)
        for t in range(T_ENV):
            env.step_act_inplace(act[t], P, None, v, a, l, done_out=d_rows[t], timeout_out=rows[t])
        check(rows[:, :, 0], d_rows, "step_act_inplace")
    env.close()

    env, _ = _env()
    rows = torch.full((T_ENV, n), 0xAA, dtype=torch.uint8, device=dev)
    _, _, _, info = env.step_n_inplace(act, done_out=d_rows, timeout_out=rows)
    check(rows, d_rows, "step_n_inplace")
    assert info["timeout"].data_ptr() == rows.data_ptr()
    with pytest.raises(AssertionError, match="timeout_out must be a contiguous uint8"):
        env.step_n_inplace(act, timeout_out=rows[0])
    with pytest.raises(AssertionError, match="timeout_out must be a contiguous uint8"):
        env.step_inplace(act[0], timeout_out=rows[0].float())
    env.close()


def test_rule_ended_envs_read_no_timeout_in_the_callers_row(gpu_device):
    """A base-height rule no robot can satisfy ends every episode at its first step.  The caller's row reads 0 beside done == 1, and
    solorl_terminate booked into the block the step was given: the engine-owned flags, filled with 0xAA, are not touched by either."""
    n, dev = 8, gpu_device
    act = _actions(n, dev)
    env, _ = _env()
    env.set_termination(base_height=10.0, min_steps=0)
    _, _, _, info = env.step_inplace(act[0])
    own = info["timeout"]                                                  # the engine-owned flags
    for t in range(1, 4):
        own.fill_(0xAA)
        row = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        _, _, d, info = env.step_inplace(act[t], timeout_out=row)
        assert bool((d == 1).all()) and bool((env.last_termination != 0).all()) and bool((row == 0).all()), t
        assert bool((own == 0xAA).all()), t
        assert info["timeout"] is row
    env.close()
    # and the time limit still comes first: with the rule off until the last step, that step is a timeout, not a rule's ending
    env, _ = _env()
    env.set_termination(base_height=10.0, min_steps=EP_LEN)
    row = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
    for t in range(EP_LEN):
        _, _, d, _ = env.step_inplace(act[t], timeout_out=row)
    assert bool((d == 1).all()) and bool((row == 1).all()) and bool((env.last_termination == 0).all())
    env.close()


# ---- rollouts
def _path_independent_policy(dev):
    """A policy every rollout path evaluates to the same bits, so that two rollouts can be compared row for row: the last layer of the
    actor and of the critic have zero weights (mean = its bias, value = its bias, whatever the order of the sums before) and the
    log-std is -60 (the noise, whose captured stream differs from the eager one, is below half an ulp of every mean)."""
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(0)
    pol = Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(dev)
    with torch.no_grad():
        pol.pi_dist.mean.weight.zero_()
        pol.pi_dist.mean.bias.uniform_(0.2, 0.9).mul_(torch.tensor([1.0, -1.0] * 6, device=dev))
        pol.base.critic[4].weight.zero_()
        pol.base.critic[4].bias.fill_(0.625)
        pol.pi_dist.logstd.fill_(-60.0)
    return pol


def _roll(dev, how, monkeypatch=None):
    """two rollouts of T = 12 on 64 envs with episode_length 5 into a storage with timeout rows -> what the storage held after each"""
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo.graphs import GraphedRollout
    from solorl_amd.ppo.train import rollout
    n = 64
    pol = _path_independent_policy(dev)
    env, obs = _env(seed=7, n=n)
    st = RolloutStorage(T_ENV, n, (76,), 12, dev, bootstrap_timeouts=True)
    st.obs[0].copy_(obs)
    st.timeouts.fill_(0xAA)
    with torch.no_grad():
        pol.act(st.obs[0])
    torch.manual_seed(11); torch.cuda.manual_seed(11)
    if how == "eager":
        run = lambda: rollout(env, pol, st, T_ENV)
    else:
        if how == "two_launch":
            monkeypatch.setenv("SOLORL_STEP_ACT", "0")
        elif how == "torch_act":
            monkeypatch.setenv("SOLORL_PPO_KERNELS", "0")
        run = GraphedRollout(env, pol, st, T_ENV, chunk=5 if how == "windows" else 0)
    out = []
    for _ in range(2):                                   # (the graph is captured at the first call and replayed at both)
        run()
        with torch.no_grad():
            nv = pol.get_value(st.obs[-1])
        st.compute_returns(nv, True, tu.GAMMA, tu.LAM)
        torch.cuda.synchronize()
        out.append({k: getattr(st, k).clone() for k in ("timeouts", "masks", "rewards", "value_preds", "returns", "actions")})
        st.reset()
    if how == "step_act":
        assert run.step_act and run.windows is None
    elif how == "windows":
        assert run.windows == [5, 5, 2]
    elif how != "eager":
        assert not run.step_act and run.windows is None
    env.close()
    return out


@pytest.fixture(scope="module")
def eager_rollouts(gpu_device):
    return _roll(gpu_device, "eager")


@pytest.mark.parametrize("how", ["step_act", "windows", "two_launch", "torch_act"])
def test_graphed_rollout_fills_timeouts_like_the_eager_loop(gpu_device, eager_rollouts, monkeypatch, how):
    """GraphedRollout in each of its forms -- the policy inside the step kernel (the default), windows of K steps in one launch, policy
    and step as two launches, the PyTorch act -- against train.rollout() on an equally seeded env: identical timeouts, masks and
    rewards, and identical returns from them, at the capture's replay and at a second one."""
    got = _roll(gpu_device, how, monkeypatch)
    for k, (g, e) in enumerate(zip(got, eager_rollouts)):
        assert bool(((e["timeouts"] == 0) | (e["timeouts"] == 1)).all())
        for name in ("timeouts", "masks", "rewards", "value_preds"):
            assert torch.equal(g[name], e[name]), (how, k, name)
        assert torch.equal(g["returns"][:-1], e["returns"][:-1]), (how, k)
        assert int(e["timeouts"].sum()) >= 64 and bool((e["masks"][1:][e["timeouts"] != 0] == 0).all())
    assert not torch.equal(eager_rollouts[0]["rewards"], eager_rollouts[1]["rewards"])     # the second rollout went on from the first


def test_bootstrapping_changes_the_returns_up_to_each_truncation_and_nothing_else(gpu_device, eager_rollouts):
    """The same rollout in a storage with and without the flags: a return differs where a truncation lies at or after its step inside
    its episode, and only there -- after an env's last truncation the two are bit-equal."""
    from solorl_amd.ppo import RolloutStorage
    e = eager_rollouts[0]
    n = e["masks"].shape[1]
    ret = {}
    for flag in (True, False):
        st = RolloutStorage(T_ENV, n, (76,), 12, gpu_device, bootstrap_timeouts=flag)
        for k in ("masks", "rewards", "value_preds"):
            getattr(st, k).copy_(e[k])
        if flag:
            st.timeouts.copy_(e["timeouts"])
        st.compute_returns(e["value_preds"][-1].clone(), True, tu.GAMMA, tu.LAM)
        ret[flag] = st.returns[:-1, :, 0].cpu()
    m, f = e["masks"][:, :, 0].cpu(), e["timeouts"][:, :, 0].cpu()
    expect = torch.zeros(T_ENV + 1, n, dtype=torch.bool)
    for t in range(T_ENV - 1, -1, -1):
        tl = (m[t + 1] == 0) & (f[t] != 0)
        expect[t] = tl | ((m[t + 1] != 0) & expect[t + 1])
    assert torch.isfinite(ret[True]).all() and torch.isfinite(ret[False]).all()
    assert torch.equal(ret[True] != ret[False], expect[:-1])
    assert bool(expect[:2 * EP_LEN].any(dim=0).all()) and not bool(expect[2 * EP_LEN:T_ENV].any())    # (two truncations per env, then a tail)
