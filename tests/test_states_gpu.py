"""Batched state access on the GPU (include/solorl.h solorl_get_states, solorl_set_states, solorl_reset_masked; SoloVecEnv.get_states,
set_states, reset_masked, push) against the per-env solorl_get_state / solorl_set_state, bit for bit, and against the fp64 oracle.

Shapes: N = 6 (two slot groups, the last one half full) and N = 130 (more than one workgroup of either kernel, ragged).  State
preparation: reset() + 5 random-action steps, so that contacts, history, dr sums and (when sorted) a shuffled slot order exist.

Contact-count sorting (SOLORL_SORT=1): rows are env ids, so a state written into ANOTHER handle lands in that handle's own slot
order.  In lane mode that is bitwise neutral; in team mode an env's sweep is specialised on the slot set of its wavefront
(tests/test_parity_gpu.py::test_lane_mode_sorting_and_team_mode_agree), so two handles only step bitwise alike while their slot orders
agree.  The sorted case that runs everything is therefore lane mode; a sorted team-mode case runs every test in which the handles
compared share their history (and with it their slot order) -- all but the "runs on from it" part of the set(all) test."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from solorl_amd.config import (default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK, TASK_POINTGOAL,
                               PRECISION_F64)
from solorl_amd.state import StateBatch, GROUP_MEMBERS, FIELD_BITS
from tests.util import check_parity_stats

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
TWIN_STEP_CASES = tuple(c for c in CASES if c != "walk12_sorted_team")      # see the module docstring
INT_MEMBERS = ("timestep", "need_reset", "contact_mask", "rng_counter")


def _cfg(case):
    robot, task, f64, H, _ = CASES[case]
    c = default_config(robot, task)
    c.num_history_stack = H
    if f64:
        c.precision = PRECISION_F64
    return c


def _make(case, N, monkeypatch, seed=5, off=3):
    from solorl_amd.vec_env import SoloVecEnv
    for k in ("SOLORL_SORT", "SOLORL_TEAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[case][4].items():
        monkeypatch.setenv(k, v)                     # (read at solorl_create)
    return SoloVecEnv(_cfg(case), N, device=DEV, seed=seed, env_id_offset=off)


def _actions(N, A, steps, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return [(torch.rand(N, A, device=DEV, generator=g) * 2 - 1).contiguous() for _ in range(steps)]


def _prepared(case, N, monkeypatch, seed=5, steps=5, act_seed=11):
    env = _make(case, N, monkeypatch, seed)
    env.reset()
    for a in _actions(N, env.act_dim, steps, act_seed):
        env.step_inplace(a)
    return env


def _rows(sb):
    return sb.bytes().cpu().numpy()


def _mask(N, k=3):
    """selected and unselected envs in every slot group of four"""
    return (torch.arange(N, device=DEV) % k == 0)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_get_states_equals_per_env_get_state_bitwise(gpu_device, monkeypatch, case, N):
    env = _prepared(case, N, monkeypatch)
    rows = _rows(env.get_states())
    assert rows.shape == (N, C.sizeof(type(env.get_state(0))))
    for i in range(N):
        assert rows[i].tobytes() == bytes(env.get_state(i)), (case, N, i)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_set_states_all_equals_per_env_set_state(gpu_device, monkeypatch, case, N):
    """B is never reset: set_states(all rows, all groups) is its reset.  Its per-env reads then equal A's; and (TWIN_STEP_CASES) three
    further steps with identical actions give bitwise equal outputs and states."""
    A = _prepared(case, N, monkeypatch)
    B = _make(case, N, monkeypatch)
    B.set_states(A.get_states())
    for i in range(N):
        assert bytes(B.get_state(i)) == bytes(A.get_state(i)), (case, N, i)
    assert np.array_equal(_rows(B.get_states()), _rows(A.get_states()))
    if case not in TWIN_STEP_CASES:
        return
    for a in _actions(N, A.act_dim, 3, seed=23):
        oa, ra, da, _ = A.step_inplace(a)
        ob, rb, db, _ = B.step_inplace(a)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states()))


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_masks_select_rows_in_both_directions(gpu_device, monkeypatch, case, N):
    A = _prepared(case, N, monkeypatch)
    full = _rows(A.get_states())
    m = _mask(N)
    sel = m.cpu().numpy()
    assert sel[:4].any() and not sel[:4].all()
    # get: unselected rows keep their prefill (a NaN pattern)
    pre = StateBatch(data=torch.full((N, full.shape[1] // 8), float("nan"), dtype=torch.float64, device=DEV))
    pre_rows = _rows(pre).copy()
    out = A.get_states(m, out=pre)
    assert out is pre
    got = _rows(out)
    assert np.array_equal(got[sel], full[sel]) and np.array_equal(got[~sel], pre_rows[~sel])
    # the same through a uint8 mask
    got8 = _rows(A.get_states(m.to(torch.uint8), out=StateBatch(data=torch.full_like(pre.data, float("nan")))))
    assert np.array_equal(got8, got)
    # set: another valid batch (a handle with another seed and other actions: the seed alone only draws a walk env's settle count, one
    # of seven), written into the selected envs only
    other = _prepared(case, N, monkeypatch, seed=99, act_seed=77).get_states()
    orow = _rows(other)
    assert (orow != full).any(axis=1).all()
    A.set_states(other, m)
    after = _rows(A.get_states())
    assert np.array_equal(after[sel], orow[sel]) and np.array_equal(after[~sel], full[~sel])
    for i in (0, 1, N - 2, N - 1):
        assert bytes(A.get_state(i)) == after[i].tobytes()


def _differs_everywhere(before, f64):
    """A batch whose every member differs from `before`, representable in the handle's arithmetic type"""
    other = before.clone()
    d = other.data[:, :-2]                                   # (the two trailing words hold the four int32 members)
    new = d * 0.5 + 0.375
    d.copy_(new if f64 else new.float().double())
    for name in INT_MEMBERS:
        getattr(other, name).add_(1)
    return other


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_field_groups_write_their_members_only(gpu_device, monkeypatch, case, N):
    A = _prepared(case, N, monkeypatch)
    f64 = CASES[case][2]
    before = A.get_states()
    other = _differs_everywhere(before, f64)
    A.set_states(other)                          # what a complete write of `other` reads back as (tau, absent joints and levels: 0)
    live = A.get_states()
    A.set_states(before)
    assert np.array_equal(_rows(A.get_states()), _rows(before))
    for group, members in GROUP_MEMBERS.items():
        for fields in (group, FIELD_BITS[group]):
            A.set_states(other, fields=fields)
            got = A.get_states()
            want = before.clone()
            for mname in members:
                getattr(want, mname).copy_(getattr(live, mname))
                assert not torch.equal(getattr(got, mname), getattr(before, mname)), (group, mname)
            assert np.array_equal(_rows(got), _rows(want)), (case, group)
            A.set_states(before)
    # several groups at once, masked
    m = _mask(N, 2)
    A.set_states(other, m, ("vel", "counters"))
    got, want = A.get_states(), before.clone()
    for mname in GROUP_MEMBERS["vel"] + GROUP_MEMBERS["counters"]:
        getattr(want, mname)[m] = getattr(live, mname)[m]
    assert np.array_equal(_rows(got), _rows(want))


def test_bad_fields_and_calls_before_reset(gpu_device, monkeypatch):
    from solorl_amd import _native
    A = _prepared("walk12", 6, monkeypatch)
    rows = A.get_states()
    p, st = C.c_void_p(rows.data.data_ptr()), A._stream()
    m = _mask(6).to(torch.uint8)
    for bad in (0, 256, 255 + 512):
        assert A.L.solorl_set_states(A._h, None, p, bad, st) == -1
        assert b"solorl_set_states" in A.L.solorl_last_error()
    assert A.L.solorl_set_states(A._h, None, None, 255, st) == -1 and A.L.solorl_get_states(A._h, None, None, st) == -1
    assert A.L.solorl_reset_masked(A._h, None, None, st) == -1
    assert np.array_equal(_rows(A.get_states()), _rows(rows))          # none of them wrote anything
    B = _make("walk12", 6, monkeypatch)                                 # never reset
    assert B.L.solorl_set_states(B._h, None, p, 2, st) == -4            # partial: fewer than all groups
    assert B.L.solorl_set_states(B._h, C.c_void_p(m.data_ptr()), p, 255, st) == -4      # partial: a mask
    assert B.L.solorl_reset_masked(B._h, C.c_void_p(m.data_ptr()), None, st) == -4
    with pytest.raises(_native.SoloRLError):
        B.push(torch.zeros(6, 3, device=DEV))
    with pytest.raises(_native.SoloRLError):
        B.step_inplace(torch.zeros(6, 12, device=DEV))
    B.get_states()                                                      # always allowed
    B.set_states(rows)                                                  # the complete write counts as the reset
    B.step_inplace(torch.zeros(6, 12, device=DEV))
    B.push(torch.zeros(6, 3, device=DEV))
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_reset_masked_equals_reset_on_the_selected_envs(gpu_device, monkeypatch, case, N):
    A, B = _prepared(case, N, monkeypatch), _prepared(case, N, monkeypatch)
    m = _mask(N)
    sel = m.cpu().numpy()
    before = _rows(B.get_states())
    assert np.array_equal(before, _rows(A.get_states()))
    cur = A.get_observation()
    obs_a = A.reset_masked(m)
    obs_b = B.reset()
    ra, rb = _rows(A.get_states()), _rows(B.get_states())
    assert np.array_equal(ra[sel], rb[sel]) and np.array_equal(ra[~sel], before[~sel])
    assert (ra[sel] != before[sel]).any(axis=1).all()
    assert torch.equal(obs_a[m], obs_b[m])
    assert torch.equal(obs_a[~m], cur[~m])                              # unselected rows: the env's current observation
    assert torch.equal(A.get_observation(), obs_a)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_push_adds_to_the_velocities_and_nothing_else(gpu_device, monkeypatch, case, N):
    A = _prepared(case, N, monkeypatch)
    f64 = CASES[case][2]
    rnd = (lambda x: x) if f64 else (lambda x: x.float().double())      # an fp32 handle rounds each double to float on write
    g = torch.Generator(device=DEV); g.manual_seed(3)
    before = A.get_states()
    dv = (torch.rand(N, 3, device=DEV, generator=g) - 0.5)
    A.push(dv)
    after = A.get_states()
    want = before.clone()
    want.lin_vel.copy_(rnd(before.lin_vel + dv))
    assert torch.equal(after.lin_vel, rnd(before.lin_vel + dv))
    assert np.array_equal(_rows(after), _rows(want))
    # linear + angular, masked
    m = _mask(N)
    dv6 = (torch.rand(N, 6, device=DEV, generator=g) - 0.5)
    A.push(dv6, m)
    after2 = A.get_states()
    want2 = after.clone()
    want2.lin_vel[m] = rnd(after.lin_vel + dv6[:, :3])[m]
    want2.ang_vel[m] = rnd(after.ang_vel + dv6[:, 3:])[m]
    assert torch.equal(after2.ang_vel[m], rnd(after.ang_vel + dv6[:, 3:])[m]) and not torch.equal(after2.ang_vel[m], after.ang_vel[m])
    assert np.array_equal(_rows(after2), _rows(want2))


@pytest.mark.parametrize("N", SIZES)
def test_push_and_step_are_capturable(gpu_device, monkeypatch, N):
    """push + step_inplace captured in one graph (a linear chain), replayed twice with fresh contents of dv and the actions, against the
    same calls issued eagerly on a twin handle."""
    A, B = _prepared("walk12", N, monkeypatch), _prepared("walk12", N, monkeypatch)
    gen = torch.Generator(device=DEV); gen.manual_seed(17)
    dv = torch.zeros(N, 6, device=DEV)
    act = torch.zeros(N, A.act_dim, device=DEV)

    def fresh():
        dv.copy_(torch.rand(N, 6, device=DEV, generator=gen) - 0.5)
        act.copy_(torch.rand(N, A.act_dim, device=DEV, generator=gen) * 2 - 1)

    fresh()                                   # warm-up outside the capture (push allocates its scratch batch at the first call)
    for e in (A, B):
        e.push(dv); e.step_inplace(act)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.push(dv)
        oa, ra, da, _ = A.step_inplace(act)
    torch.cuda.synchronize()
    assert np.array_equal(_rows(A.get_states()), _rows(B.get_states()))      # capturing ran nothing
    for _ in range(2):
        fresh()
        graph.replay()
        B.push(dv)
        ob, rb, db, _ = B.step_inplace(act)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states()))


def test_capture_on_a_sorted_handle_with_an_even_number_of_steps(gpu_device, monkeypatch):
    """Contact-count sorting ping-pongs two state buffers on the host side of solorl_step, and a captured call holds the buffer that
    was current when it was issued: push + an EVEN number of steps leaves the handle on the buffer the
    graph starts from, so the graph replays correctly.  Lane mode, where sorting is bitwise neutral, against an eager twin."""
    case, N = "walk12_sorted_lane", 130
    A, B = _prepared(case, N, monkeypatch), _prepared(case, N, monkeypatch)
    gen = torch.Generator(device=DEV); gen.manual_seed(29)
    dv = torch.zeros(N, 3, device=DEV)
    act = torch.zeros(2, N, A.act_dim, device=DEV)

    def fresh():
        dv.copy_(torch.rand(N, 3, device=DEV, generator=gen) - 0.5)
        act.copy_(torch.rand(2, N, A.act_dim, device=DEV, generator=gen) * 2 - 1)

    def calls(e):
        e.push(dv)
        e.step_inplace(act[0])
        return e.step_inplace(act[1])

    fresh()
    calls(A); calls(B)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa, ra, da, _ = calls(A)
    for _ in range(2):
        fresh()
        graph.replay()
        ob, rb, db, _ = calls(B)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states()))


def test_teleport_and_push_against_the_oracle(gpu_device, monkeypatch):
    """Solo12 pointgoal fp32, 32 envs, one control step deep: half of the envs are moved by +-0.3 m in xy with `potential` rewritten
    (pose + task groups), all are pushed by up to 0.5 m/s; the oracle is loaded from get_states() and both step.  Bounds as
    tests/test_parity_gpu.py::test_step_matches_oracle_resynced: per-env joint error median < 1e-4 rad, p90 < 1e-3 rad; reward
    difference (it carries `progress` = the change of the distance to the goal FROM THE NEW POSITION, times 60) median < 1e-3 --
    over all envs and over the moved ones alone (a potential left at the old position would put up to 18 on each of those)."""
    from solorl_amd.vec_env import SoloVecEnv
    from oracle.oracle_py import Oracle
    for k in ("SOLORL_SORT", "SOLORL_TEAM"):
        monkeypatch.delenv(k, raising=False)
    N = 32
    c = default_config(ROBOT_SOLO12, TASK_POINTGOAL); c.num_history_stack = 1
    env = SoloVecEnv(c, N, device=DEV, seed=3)
    orc = Oracle(c, N, seed=3, threads=min(16, len(os.sched_getaffinity(0))))
    env.reset(); orc.reset()
    acts = _actions(N, 12, 6, seed=2)
    for a in acts[:5]:
        env.step_inplace(0.3 * a)
    g = torch.Generator(device=DEV); g.manual_seed(8)
    moved = torch.arange(N, device=DEV) % 2 == 0
    s = env.get_states()
    shift = torch.where(torch.rand(N, 2, device=DEV, generator=g) < 0.5, -0.3, 0.3).double()
    s.pos[:, :2] += shift
    s.potential.copy_(((s.pos[:, :2] - s.goal) ** 2).sum(dim=1).sqrt())
    env.set_states(s, moved, ("pose", "task"))
    env.push((torch.rand(N, 3, device=DEV, generator=g) * 2 - 1) * 0.5)
    loaded = env.get_states()
    assert torch.equal(loaded.pos[moved], s.pos[moved].float().double()) and not torch.equal(loaded.pos[~moved], s.pos[~moved].float().double())
    for i in range(N):
        orc.set_state(i, loaded.env_state(i))
    a = acts[5]
    obs, rew, done, _ = env.step(a)
    oobs, orew, odone, _ = orc.step(a.cpu().numpy().astype(np.float64))
    after = env.get_states()
    done = done.cpu().numpy() != 0; rew = rew.cpu().numpy()[:, 0]
    ok = ~done & ~(np.asarray(odone) != 0)
    assert ok.sum() >= N - 4, ok.sum()
    q = after.q.cpu().numpy()
    dq = np.array([np.abs(q[i] - np.array(orc.get_state(i).q)).max() for i in range(N)])[ok]
    dr = np.abs(rew - orew)
    mv = moved.cpu().numpy()
    stats = check_parity_stats("states_teleport_push/robot1_task2", dq)
    print("teleport+push: reward diff median %.3e (moved envs %.3e), max %.3e" % (np.median(dr[ok]), np.median(dr[ok & mv]), dr[ok].max()))
    assert np.median(dq) < 1e-4 and np.percentile(dq, 90) < 1e-3, stats
    assert np.median(dr[ok]) < 1e-3 and np.median(dr[ok & mv]) < 1e-3
    # the moved envs' progress is measured from the new position: |progress| is a step's travel, far below the 0.3 m jump
    assert after.progress[moved & torch.from_numpy(ok).to(DEV)].abs().max().item() < 0.1
