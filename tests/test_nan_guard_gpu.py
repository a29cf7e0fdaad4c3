"""The non-finite-state guard of the step kernels, fired on purpose (include/solorl.h: "A per-env numeric failure (NaN/Inf state) is NOT an
error: the env is force-terminated, reset and counted in info.nan_reset").  Every other test of the suite asserts nan_reset == 0.

Two identically seeded handles, A (poisoned) and B (clean), Solo12 walk unless stated, one history level, N = 67: 17 team wavefronts of
four envs, the last one ragged.  After ~10 common warm-up steps env `e` of A is poisoned -- a NaN in its action row (what a diverged
policy hands over: the clip leaves NaN NaN), or a non-finite / out-of-range member written with set_states -- and both handles step
with the same actions.  Then B.reset_masked({e}) supplies the exact reference: the guard's reset is the same snapshot copy from the env's
own Philox counter, no arithmetic, so A's row of `e` must equal B's BITWISE in every execution form.

What the rest of the batch may show:
  * an env outside e's wavefront (team mode: i // 4 != e // 4; lane mode: every other env) never meets the poisoned values: bitwise B's;
  * e's three wavefront-mates in team mode share the LDS rows, the PGS exit ballot and the sweep variant with it.  An env's sweep is
    specialised on its wavefront's slot set (tests/test_parity_gpu.py::test_lane_mode_sorting_and_team_mode_agree), so they are NOT
    bitwise B's and this file does not claim it: one step from bitwise-equal states their joint angles are held to the one-step bounds of
    tests/test_parity_gpu.py::test_step_matches_oracle_resynced -- every sample < 1e-3 rad, median < 1e-4 rad -- and their done /
    nan_reset / ep_stats must be B's exactly.

The same poisons run through the kernel's sub-step code on the CPU under the sanitizers first (tests/test_host_nonfinite.py)."""
import numpy as np
import pytest
import torch

from solorl_amd.config import (default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK, TASK_POINTGOAL, PRECISION_F64)
from tests.util import check_parity_stats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 67
WARMUP = 10
NAN, INF = float("nan"), float("inf")
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")
#        form       environment at solorl_create      f64  helper_wave  lanes_per_env
FORMS = {"team":    ({},                              0,   1,           16),
         "classic": ({"SOLORL_HELPER_WAVE": "0"},     0,   0,           16),
         "lane":    ({"SOLORL_TEAM": "0"},            0,   0,           1),
         "f64":     ({},                              1,   0,           16)}
CONFIGS = {"walk12": (ROBOT_SOLO12, TASK_WALK), "stand8": (ROBOT_SOLO8, TASK_STAND), "pointgoal12": (ROBOT_SOLO12, TASK_POINTGOAL)}
# position of the poisoned env(s): slot k of one full wavefront (chosen below), the ragged wavefront's last valid team, two in one wavefront
POSITIONS = {"slot0": (0,), "slot1": (1,), "slot2": (2,), "slot3": (3,), "last": None, "pair": (0, 2)}


def _poison_action(env, act, es):
    act = act.clone()
    act[list(es), 5] = NAN
    return act


def _poison_state(member, group, index, value):
    def apply(env, act, es):
        s = env.get_states()
        getattr(s, member)[list(es), index] = value
        m = torch.zeros(N, dtype=torch.bool, device=DEV); m[list(es)] = True
        env.set_states(s, m, group)
        return act
    return apply


POISONS = {"action": _poison_action,
           "vel_inf": _poison_state("lin_vel", "vel", 2, INF),
           "q_nan": _poison_state("q", "joint_pos", 7, NAN),
           "quat_x_nan": _poison_state("quat", "pose", 0, NAN),      # the guard sums qw, not qx: this must spread within the step
           "pos_1e31": _poison_state("pos", "pose", 0, 1e31)}        # finite (as a float too), above the guard's 1e30 threshold


def _bits(x):
    """NaN-proof equality: float tensors compared as their words"""
    return x.view(torch.int32) if x.dtype == torch.float32 else (x.view(torch.int64) if x.dtype == torch.float64 else x)


def _same(x, y):
    return torch.equal(_bits(x.contiguous()), _bits(y.contiguous()))


def _make(monkeypatch, form, cfg, seed=5):
    from solorl_amd.vec_env import SoloVecEnv
    envvars, f64, helper, lanes = FORMS[form]
    robot, task = CONFIGS[cfg]
    c = default_config(robot, task); c.num_history_stack = 1
    if f64:
        c.precision = PRECISION_F64
    for k in ("SOLORL_SORT", "SOLORL_TEAM", "SOLORL_HELPER_WAVE", "SOLORL_POISON_LDS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)                      # (read at solorl_create)
    env = SoloVecEnv(c, N, device=DEV, seed=seed, env_id_offset=3)
    for k in envvars:
        monkeypatch.delenv(k)
    assert env.get_property("lanes_per_env") == lanes and env.get_property("helper_wave") == helper and env.get_property("f64") == f64
    return env


def _pair(monkeypatch, form, cfg, gen):
    """A and B, reset and warmed up with common actions: bitwise equal states, contacts, history and dr sums in place"""
    A, B = _make(monkeypatch, form, cfg), _make(monkeypatch, form, cfg)
    assert torch.equal(A.reset(), B.reset())
    for _ in range(WARMUP):
        a = (torch.rand(N, A.act_dim, device=DEV, generator=gen) * 2 - 1) * 0.5
        A.step_inplace(a); B.step_inplace(a)
    assert _same(A.get_states().data, B.get_states().data)
    return A, B


def _out(step_result, env):
    o, r, d, info = step_result
    return dict(obs=o.clone(), rew=r.clone().view(-1), done=d.clone(), info={k: v.clone() for k, v in info.items()}, ep=env._ep_stats.clone())


def _choose(pos, done_b):
    """The poisoned envs for a position, from B's (clean) done flags of the step: a full wavefront none of whose envs ends its episode in
    this very step (an env that falls in the same step would be reset twice in B), never the first or the last one."""
    done_b = done_b.cpu().numpy() != 0
    if POSITIONS[pos] is None:
        assert not done_b[64:67].any()
        return (66,)
    for w in range(8, 16):
        if not done_b[4 * w:4 * w + 4].any():
            return tuple(4 * w + k for k in POSITIONS[pos])
    raise AssertionError("no quiet wavefront")


def _check_poisoned_step(name, A, B, es, a_out, b_out, ep_before):
    """`a_out` / `b_out`: the outputs of the step in which A's envs `es` were poisoned.  Resets `es` in B (reset_masked)."""
    team = A.get_property("lanes_per_env") == 16
    f64 = A.get_property("f64") == 1
    es = list(es)
    sb_step = B.get_states()
    assert torch.isfinite(sb_step.data[es, :-2]).all() and not b_out["done"][es].any()       # B's rows of `es` are finite and alive
    m = torch.zeros(N, dtype=torch.bool, device=DEV); m[es] = True
    B.reset_masked(m)
    sa, sb = A.get_states(), B.get_states()
    obs_b = B.get_observation()
    ia = a_out["info"]
    # ---- the poisoned envs
    for e in es:
        assert a_out["done"][e].item() == 1 and a_out["rew"][e].item() == 0.0, (e, a_out["done"][e].item(), a_out["rew"][e].item())
        assert ia["timeout"][e].item() == 0 and ia["success"][e].item() == 0 and ia["nan_reset"][e].item() == 1, e
        assert a_out["ep"][9, e].item() == ep_before[9, e].item() + 1.0
        assert _same(a_out["ep"][:9, e], ep_before[:9, e]), e                # not counted among the finished episodes
        assert torch.isfinite(a_out["obs"][e]).all(), e
        assert _same(sa.data[e], sb.data[e]), (e, (sa.data[e] != sb.data[e]).nonzero().flatten().tolist())     # the whole row, bitwise
        assert _same(a_out["obs"][e], obs_b[e]), e
        assert sa.timestep[e].item() == 0 and sa.rng_counter[e].item() == sb_step.rng_counter[e].item() + (2 if A.cfg.task == TASK_POINTGOAL else 1)
    assert int(ia["nan_reset"].sum()) == len(es)
    # ---- everybody who cannot have met the poisoned values: bitwise B's
    idx = np.arange(N)
    far = torch.from_numpy(~np.isin(idx // 4 if team else idx, [e // 4 if team else e for e in es])).to(DEV)
    assert int(far.sum()) == (N - 4 if team and es[0] < 64 else N - 3 if team else N - len(es))
    assert _same(a_out["obs"][far], b_out["obs"][far]) and _same(a_out["rew"][far], b_out["rew"][far]) and _same(a_out["done"][far], b_out["done"][far])
    assert _same(sa.data[far], sb.data[far])
    for f in INFO:
        assert _same(ia[f][far], b_out["info"][f][far]), f
    assert _same(a_out["ep"][:, far], b_out["ep"][:, far])
    # ---- the wavefront-mates (team mode): one step from bitwise-equal states
    if team:
        mates = [i for i in range(4 * (es[0] // 4), min(N, 4 * (es[0] // 4) + 4)) if i not in es]
        assert len(mates) == (2 if len(es) == 2 or es[0] >= 64 else 3)
        nq = A.act_dim
        dq = (sa.q[mates, :nq] - sb.q[mates, :nq]).abs().max(dim=1).values.cpu().numpy()
        assert np.isfinite(sa.data[mates, :-2].cpu().numpy()).all() and torch.isfinite(a_out["obs"][mates]).all()
        check_parity_stats("nan_guard/" + name, dq, floor=1e-13 if f64 else 1e-7)
        assert dq.max() < 1e-3 and np.median(dq) < 1e-4, dq
        assert _same(a_out["done"][mates], b_out["done"][mates]) and _same(ia["nan_reset"][mates], b_out["info"]["nan_reset"][mates])
        assert _same(a_out["ep"][:, mates], b_out["ep"][:, mates])
    return far


def _run_on(A, B, gen, far, steps=5):
    """`steps` more steps with common finite actions: lane mode bitwise; team mode finite, no further guard reset (and, the wavefronts
    being independent, still bitwise outside the poisoned one)"""
    team = A.get_property("lanes_per_env") == 16
    for _ in range(steps):
        a = (torch.rand(N, A.act_dim, device=DEV, generator=gen) * 2 - 1) * 0.5
        x, y = _out(A.step_inplace(a), A), _out(B.step_inplace(a), B)
        assert int(x["info"]["nan_reset"].sum()) == 0 and torch.isfinite(x["obs"]).all() and torch.isfinite(x["rew"]).all()
        sel = far if team else slice(None)
        assert _same(x["obs"][sel], y["obs"][sel]) and _same(x["rew"][sel], y["rew"][sel]) and _same(x["done"][sel], y["done"][sel])
    sa, sb = A.get_states(), B.get_states()
    assert torch.isfinite(sa.data[:, :-2]).all()
    assert _same(sa.data[far] if team else sa.data, sb.data[far] if team else sb.data)


#        form       config         position  poison            every value of every axis at least once; every form sees the NaN action
CASES = [("team",    "walk12",      "slot0", "action"),      # and a set_states poison; every form sees a pair, and the ragged wavefront
         ("team",    "walk12",      "slot1", "vel_inf"),     # or a single env
         ("team",    "walk12",      "slot2", "q_nan"),
         ("team",    "walk12",      "slot3", "quat_x_nan"),
         ("team",    "walk12",      "last",  "pos_1e31"),
         ("team",    "walk12",      "pair",  "action"),
         ("classic", "walk12",      "slot1", "action"),
         ("classic", "walk12",      "last",  "q_nan"),
         ("classic", "walk12",      "pair",  "vel_inf"),
         ("lane",    "walk12",      "slot2", "action"),
         ("lane",    "walk12",      "last",  "quat_x_nan"),
         ("lane",    "walk12",      "pair",  "pos_1e31"),
         ("f64",     "walk12",      "slot3", "action"),
         ("f64",     "walk12",      "slot0", "pos_1e31"),
         ("f64",     "walk12",      "pair",  "quat_x_nan"),
         ("team",    "stand8",      "slot1", "q_nan"),
         ("lane",    "stand8",      "slot3", "action"),
         ("team",    "pointgoal12", "slot2", "pos_1e31"),    # goal, potential and rng_counter are part of the row compared bitwise
         ("lane",    "pointgoal12", "slot0", "action")]


@pytest.mark.parametrize("form,cfg,pos,poison", CASES)
def test_nan_guard_resets_the_env_and_nothing_else(gpu_device, monkeypatch, form, cfg, pos, poison):
    gen = torch.Generator(device=DEV); gen.manual_seed(21)
    A, B = _pair(monkeypatch, form, cfg, gen)
    act = (torch.rand(N, A.act_dim, device=DEV, generator=gen) * 2 - 1) * 0.5
    ep_before = A._ep_stats.clone()
    b_out = _out(B.step_inplace(act), B)                 # (B first: its done flags choose the wavefront, see _choose)
    es = _choose(pos, b_out["done"])
    act_a = POISONS[poison](A, act, es)
    a_out = _out(A.step_inplace(act_a), A)
    far = _check_poisoned_step("%s_%s_%s_%s" % (form, cfg, pos, poison), A, B, es, a_out, b_out, ep_before)
    _run_on(A, B, gen, far)
    torch.cuda.synchronize()
    A.close(); B.close()


def test_nan_guard_inside_a_step_n_window(gpu_device, monkeypatch):
    """solorl_step_n, K = 4, the NaN action in row [1][e]: per-step info rows [K][N]; the env continues from its reset inside the window.
    Against 4 single steps of a twin handle given the same (poisoned) actions, bitwise as
    tests/test_step_n_gpu.py::test_step_n_equals_k_single_steps_bitwise -- and, step by step, against the clean handle B."""
    K = 4
    gen = torch.Generator(device=DEV); gen.manual_seed(22)
    A, B = _pair(monkeypatch, "team", "walk12", gen)
    gen2 = torch.Generator(device=DEV); gen2.manual_seed(22)
    R, _B2 = _pair(monkeypatch, "team", "walk12", gen2)          # R: the single-step twin of A
    _B2.close()
    assert A.get_property("step_n_one_launch") == 1
    acts = (torch.rand(K, N, 12, device=DEV, generator=gen) * 2 - 1) * 0.5
    ep_before = A._ep_stats.clone()
    b_rows = [_out(B.step_inplace(acts[0].contiguous()), B)]
    b_rows.append(_out(B.step_inplace(acts[1].contiguous()), B))
    es = _choose("slot1", b_rows[1]["done"] | b_rows[0]["done"])
    e = es[0]
    pa = acts.clone(); pa[1, e, 5] = NAN
    o, r, d, info = A.step_n_inplace(pa)
    got = dict(obs=o.clone(), rew=r.clone(), done=d.clone(), info={k: v.clone() for k, v in info.items()})
    ep_after_a = A._ep_stats.clone()
    # ---- against K single steps with the same actions: every output of every step, bitwise
    for k in range(K):
        w = _out(R.step_inplace(pa[k].contiguous()), R)
        assert _same(got["obs"][k], w["obs"]) and _same(got["rew"][k], w["rew"]) and _same(got["done"][k], w["done"]), k
        for f in INFO:
            assert _same(got["info"][f][k], w["info"][f]), (k, f)
    assert _same(ep_after_a, R._ep_stats) and _same(A.get_states().data, R.get_states().data)
    # ---- the poisoned step = row 1, with the assertions of the single-step test (R is bitwise A: its step-1 state is what they need)
    assert got["info"]["nan_reset"].shape == (K, N) and int(got["info"]["nan_reset"].sum()) == 1 and got["info"]["nan_reset"][1, e].item() == 1
    assert got["done"][1, e].item() == 1 and got["rew"][1, e].item() == 0.0 and got["info"]["timeout"][1, e].item() == 0 and got["info"]["success"][1, e].item() == 0
    assert torch.isfinite(got["obs"]).all() and torch.isfinite(got["rew"]).all()
    assert got["info"]["episode_length"][2, e].item() == 1 and got["info"]["episode_length"][3, e].item() == 2      # it went on from its reset
    assert not got["done"][2:, e].any()
    assert ep_after_a[9, e].item() == ep_before[9, e].item() + 1.0 and _same(ep_after_a[:9, e], ep_before[:9, e])
    m = torch.zeros(N, dtype=torch.bool, device=DEV); m[e] = True
    B.reset_masked(m)
    assert _same(got["obs"][1, e], B.get_observation()[e])
    # ---- envs outside e's wavefront: bitwise B's through the whole window
    far = torch.from_numpy(np.arange(N) // 4 != e // 4).to(DEV)
    for k in (2, 3):
        b_rows.append(_out(B.step_inplace(acts[k].contiguous()), B))
    for k in range(K):
        assert _same(got["obs"][k][far], b_rows[k]["obs"][far]) and _same(got["rew"][k][far], b_rows[k]["rew"][far]), k
        assert _same(got["done"][k][far], b_rows[k]["done"][far]), k
    assert _same(A.get_states().data[far], B.get_states().data[far])
    torch.cuda.synchronize()
    A.close(); B.close(); R.close()


def _policy_and_params():
    from solorl_amd.ppo.fused import policy_params
    from tests.test_step_n_gpu import _policy
    pol = _policy(torch.device(DEV), 76, 12)
    return pol, policy_params(pol)


def _policy_outputs_match(P, obs, noise, v, a, l, rows):
    """value / action / log-prob of `rows` against solorl_policy_act on the same observation rows, within the bounds of
    tests/test_train_gpu.py::test_step_act_equals_step_then_policy_act"""
    from solorl_amd.ppo.fused import policy_act
    v1, a1, l1 = torch.empty(N, 1, device=DEV), torch.empty(N, 12, device=DEV), torch.empty(N, 1, device=DEV)
    policy_act(P, obs.contiguous(), noise, v1, a1, l1)
    for x, y, bound in ((v1, v, 5e-6), (a1, a, 5e-6), (l1, l, 2e-5)):
        x, y = x[rows], y[rows]
        assert torch.isfinite(y).all()
        assert float(((x - y).abs() / (1.0 + y.abs())).max()) < bound


@pytest.mark.parametrize("poison", ["action", "noise"])
def test_nan_guard_in_step_act(gpu_device, monkeypatch, poison):
    """solorl_step_act: the NaN action -- and NaN in the noise row of e, which makes the policy tail itself produce the NaN action that
    trips the guard one step later.  The policy outputs of every other env stay within the step_act bounds; e's value is finite and its
    observation is the reset row."""
    gen = torch.Generator(device=DEV); gen.manual_seed(23)
    A, B = _pair(monkeypatch, "team", "walk12", gen)
    pol, P = _policy_and_params()
    assert A.step_act_supported(P)
    act = (torch.rand(N, 12, device=DEV, generator=gen) * 2 - 1) * 0.5
    noise = torch.randn(N, 12, device=DEV, generator=gen)

    def bufs():
        return torch.full((N, 1), 7.0, device=DEV), torch.full((N, 12), 7.0, device=DEV), torch.full((N, 1), 7.0, device=DEV)

    others = torch.ones(N, dtype=torch.bool, device=DEV)
    if poison == "noise":
        # step 0: clean actions, NaN noise for e.  B runs its two steps first: its done flags choose the wavefront (see _choose)
        noise1 = torch.randn(N, 12, device=DEV, generator=gen)
        vb0, ab0, lb0 = bufs()
        y0 = _out(B.step_act_inplace(act, P, noise, vb0, ab0, lb0), B)
        ep_b0 = B._ep_stats.clone()
        vb, ab, lb = bufs()
        b_out = _out(B.step_act_inplace(ab0.clone(), P, noise1, vb, ab, lb), B)
        es = _choose("slot1", y0["done"] | b_out["done"])
        e = es[0]
        na = noise.clone(); na[e, 2] = NAN
        va, aa, la = bufs()
        x0 = _out(A.step_act_inplace(act, P, na, va, aa, la), A)
        assert _same(x0["obs"], y0["obs"]) and int(x0["info"]["nan_reset"].sum()) == 0      # nothing has happened to the physics yet
        others[e] = False
        assert torch.isnan(aa[e, 2]) and torch.isfinite(va[e]).all() and _same(aa[others], ab0[others]) and _same(va, vb0)
        _policy_outputs_match(P, x0["obs"], noise, va, aa, la, others)
        act_a, noise = aa.clone(), noise1
        ep_before = A._ep_stats.clone()
        assert _same(ep_before, ep_b0)
    else:
        ep_before = A._ep_stats.clone()
        vb, ab, lb = bufs()
        b_out = _out(B.step_act_inplace(act, P, noise, vb, ab, lb), B)
        es = _choose("slot2", b_out["done"])
        act_a = _poison_action(A, act, es)
    va, aa, la = bufs()
    a_out = _out(A.step_act_inplace(act_a, P, noise, va, aa, la), A)
    far = _check_poisoned_step("step_act_%s" % poison, A, B, es, a_out, b_out, ep_before)
    # the policy tail on the observations this step produced: every env, e with its reset row included
    assert torch.isfinite(va).all() and torch.isfinite(aa).all() and torch.isfinite(la).all()
    _policy_outputs_match(P, a_out["obs"], noise, va, aa, la, torch.ones(N, dtype=torch.bool, device=DEV))
    assert _same(va[far], vb[far]) and _same(aa[far], ab[far]) and _same(la[far], lb[far])
    torch.cuda.synchronize()
    A.close(); B.close()


def test_nan_guard_inside_a_rollout_window(gpu_device, monkeypatch):
    """solorl_rollout, K = 4, NaN in noise row [1][e]: the policy's own action of row 1 is NaN and trips the guard in step 1.  Against
    4 x solorl_step_act closed the same way, bitwise, as tests/test_step_n_gpu.py::test_rollout_equals_k_step_act_bitwise -- and
    against a clean twin B: observation row [1][e] is B's reset_masked row, envs outside e's wavefront are B's bitwise in every row."""
    from tests.test_step_n_gpu import _closed_ref, _closed_cand
    K = 4
    gen = torch.Generator(device=DEV); gen.manual_seed(24)
    A, R = _pair(monkeypatch, "team", "walk12", gen)             # A: one launch; R: K x step_act
    gen2 = torch.Generator(device=DEV); gen2.manual_seed(24)
    B, _B2 = _pair(monkeypatch, "team", "walk12", gen2)          # B: the clean twin
    _B2.close()
    pol, P = _policy_and_params()
    assert A.rollout_supported(P)
    a0 = (torch.rand(N, 12, device=DEV, generator=gen) * 2 - 1) * 0.5
    clean = torch.randn(K + 1, N, 12, device=DEV, generator=gen)
    # B first, two steps by hand: its done flags choose the wavefront, and it stops behind the step that is poisoned in A
    val, lp = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    act1, act2 = torch.empty(N, 12, device=DEV), torch.empty(N, 12, device=DEV)
    b0 = _out(B.step_act_inplace(a0, P, clean[1].contiguous(), val, act1, lp), B)
    b1 = _out(B.step_act_inplace(act1, P, clean[2].contiguous(), val, act2, lp), B)
    e = _choose("slot2", b0["done"] | b1["done"])[0]
    m = torch.zeros(N, dtype=torch.bool, device=DEV); m[e] = True
    B.reset_masked(m)
    reset_row = B.get_observation()[e].clone()
    noise = clean.clone()
    noise[1, e, 4] = NAN
    ep_before = A._ep_stats.clone()
    want, got = _closed_ref(R, P, a0, noise, K, 1), _closed_cand(A, P, a0, noise, K, 1)
    for k in ("obs", "rew", "done", "act", "val", "lp"):
        assert _same(want[k], got[k]), k
    assert _same(A._ep_stats, R._ep_stats) and _same(A.get_states().data, R.get_states().data)
    assert torch.isnan(got["act"][1, e, 4]) and torch.isfinite(got["val"][1:]).all()
    assert torch.isfinite(got["obs"]).all() and torch.isfinite(got["rew"]).all()
    assert not got["done"][0, e].item() and got["done"][1, e].item() == 1 and got["rew"][1, e].item() == 0.0 and not got["done"][2:, e].any()
    assert torch.isfinite(got["act"][2:]).all() and torch.isfinite(got["lp"][2:]).all()          # the policy on the reset row: finite again
    assert A._ep_stats[9, e].item() == ep_before[9, e].item() + 1.0 and _same(A._ep_stats[:9, e], ep_before[:9, e])
    assert float(A._ep_stats[9].sum() - ep_before[9].sum()) == 1.0
    # ---- against the clean twin
    assert _same(got["obs"][1, e], reset_row)
    far = torch.from_numpy(np.arange(N) // 4 != e // 4).to(DEV)
    for k, b in enumerate((b0, b1)):
        assert _same(got["obs"][k][far], b["obs"][far]) and _same(got["rew"][k][far], b["rew"][far]) and _same(got["done"][k][far], b["done"][far]), k
    assert _same(got["act"][1][far], act1[far]) and _same(got["act"][2][far], act2[far])
    torch.cuda.synchronize()
    A.close(); R.close(); B.close()
