"""Shared by tests/test_shape_host.py and tests/test_shape_gpu.py: the seeded inputs of the solorl_shape_reward checks, the stand-alone
host program (tests/host/shape_main.cpp) and the reference its outputs are compared with -- a numpy restatement of the term table of
include/solorl.h, which takes the feet's points, velocities and forces from the solorl_kinematics host rows (tests/kin_util.py) and
nothing from the engine's source."""
import ctypes as C
import functools
import os
import tempfile
import types

import numpy as np

from solorl_amd.config import EnvState
from solorl_amd.shaping import EnvShape, ShapeParams, TERMS, ROW_WORDS, SHAPE_TERMS, EP_FIELDS, make_params
from tests import kin_util as ku
from tests.host_util import run_host

SEED = 20250307      # gives the coverage tests/test_shape_host.py asserts (every term, first contact, collision, foot force)
FOOT_PRIMS = (13, 15, 17, 19)
STATE_WORDS = C.sizeof(EnvState) // 8
SW = {name: getattr(EnvState, name).offset // 8 for name, _ in EnvState._fields_}       # member -> first 8-byte word of the state row
MW = {name: getattr(EnvShape, name).offset // 8 for name, _ in EnvShape._fields_}       # member -> first 8-byte word of the memory row
F_MASK, F_DONE, F_REWARD, F_TERMS, F_EP = 1, 2, 4, 8, 16
F_ALL = F_DONE | F_REWARD | F_TERMS | F_EP


# ---------------------------------------------------------------- the host program
shape_main = functools.partial(ku.host_main, "shape_main")


def run_shape_main(c, flags=F_ALL, mask=None, states=None, sanitize=False):
    """The host program on case ``c`` (``states``: rows to use instead of c.states) -> (mem [n, 45], reward [n] f32, terms [n, 16],
    ep [17, n]) as the call leaves them; an array whose flag is not set is passed as a null pointer and comes back as it went in."""
    exe = shape_main(sanitize)
    n = c.n
    if mask is not None:
        flags |= F_MASK
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(bytes(c.cfg)); f.write(bytes(c.params)); f.write(np.array([n, flags], np.int32).tobytes())
            for a in (c.states if states is None else states, c.actions, c.mem, c.reward, c.terms, c.ep,
                      np.ones(n, np.uint8) if mask is None else np.asarray(mask, np.uint8), c.done):
                f.write(np.ascontiguousarray(a).tobytes())
        run_host(exe, (fin, fout), timeout=120)
        raw = open(fout, "rb").read()
    o = 0
    out = []
    for shape, dt in (((n, ROW_WORDS), np.float64), ((n,), np.float32), ((n, SHAPE_TERMS), np.float64), ((EP_FIELDS, n), np.float64)):
        k = int(np.prod(shape)) * np.dtype(dt).itemsize
        out.append(np.frombuffer(raw[o:o + k], dt).reshape(shape).copy())
        o += k
    assert o == len(raw)
    return tuple(out)


# ---------------------------------------------------------------- inputs
def mem_ints(mem):
    """(prev_contact [n], valid [n]) int32 views of memory rows [n, 45]"""
    ints = mem.view(np.int32).reshape(mem.shape[0], 2 * ROW_WORDS)
    return ints[:, 2 * MW["prev_contact"]], ints[:, 2 * MW["prev_contact"] + 1]


def state_rows(states):
    """sequence of EnvState -> float64 [n, 255] (bytes as they are)"""
    return np.frombuffer(b"".join(bytes(s) for s in states), np.float64).reshape(len(states), STATE_WORDS).copy()


def env_states(rows):
    return [EnvState.from_buffer_copy(np.ascontiguousarray(r).tobytes()) for r in rows]


def contact_masks(rows):
    return rows.view(np.int32).reshape(rows.shape[0], 2 * STATE_WORDS)[:, EnvState.contact_mask.offset // 4]


_CASES = {}


def case(robot, n=64):
    """Seeded inputs of one call on n rows -- the 64 states of kin_util.inputs(robot, 0) (32 random poses, 32 oracle rollout states
    with contacts), repeated as needed, with torques U(-3, 3) in the rows' tau; actions U(-1.5, 1.5); random valid memory rows
    (valid in {0, 1}, prev_contact random, air_time in [0, 0.5], ep_sum random); random done flags, at least 8 set and 8 clear among
    every 64; all weights non-zero; foot_force_max from the inputs' own force range.  Computed once per process, never modified."""
    if (robot, n) not in _CASES:
        cfg, states = ku.inputs(robot, 0)
        nq = cfg.n_joints
        rng = np.random.default_rng(SEED + 1000 * robot + n)
        rows = state_rows(states)[np.arange(n) % len(states)]
        rows[:, SW["tau"]:SW["tau"] + nq] = rng.uniform(-3, 3, (n, nq))
        mem = np.zeros((n, ROW_WORDS))
        mem[:, MW["prev_action"]:MW["prev_action"] + 12] = rng.uniform(-1.5, 1.5, (n, 12))
        mem[:, MW["prev_qd"]:MW["prev_qd"] + 12] = rng.uniform(-30, 30, (n, 12))
        mem[:, MW["air_time"]:MW["air_time"] + 4] = rng.uniform(0, 0.5, (n, 4))
        mem[:, MW["ep_sum"]:MW["ep_sum"] + SHAPE_TERMS] = rng.uniform(-5, 5, (n, SHAPE_TERMS))
        pc, valid = mem_ints(mem)
        pc[:] = rng.integers(0, 16, n)
        valid[:] = rng.integers(0, 2, n)
        done = (rng.random(n) < 0.25).astype(np.uint8)
        assert 8 <= int(done[:64].sum()) <= 56 or n < 64, done.sum()
        cm = contact_masks(rows)
        force = np.where((cm[:, None] >> np.array(FOOT_PRIMS)) & 1, rows[:, [SW["lambda_prev"] + p for p in FOOT_PRIMS]] / cfg.sim_dt, 0.0)
        weights = {name: float(w) for name, w in zip(TERMS, rng.uniform(0.5, 2.0, SHAPE_TERMS) * rng.choice([-1.0, 1.0], SHAPE_TERMS))}
        params = make_params(weights, base_height_target=0.24, foot_clearance_target=0.06, foot_force_max=0.5 * float(force[done == 0].max()),
                             air_time_target=0.25, cmd_lin_vel=(0.5, 0.1), cmd_yaw_rate=0.3, tracking_sigma=0.25)
        _CASES[(robot, n)] = types.SimpleNamespace(
            robot=robot, n=n, cfg=cfg, params=params, states=rows, actions=rng.uniform(-1.5, 1.5, (n, nq)).astype(np.float32), mem=mem, done=done,
            reward=rng.uniform(-2, 2, n).astype(np.float32), terms=rng.uniform(-1, 1, (n, SHAPE_TERMS)), ep=rng.uniform(0, 3, (EP_FIELDS, n)))
        for a in vars(_CASES[(robot, n)]).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _CASES[(robot, n)]


_KIN = {}


def kin_rows(c):
    """the solorl_kinematics host rows of the case's states (tests/host/rows_main.cpp), once per case"""
    if (c.robot, c.n) not in _KIN:
        base = ku.run_kin_main(c.cfg, env_states(case(c.robot, c.n).states[:64]))     # (the seeded rows, whatever a test has poisoned in a copy)
        _KIN[(c.robot, c.n)] = base[np.arange(c.n) % 64]
    return _KIN[(c.robot, c.n)]


# ---------------------------------------------------------------- the reference: the term table in numpy
def reference_terms(c, i, kin):
    """(terms [16], first_f [4], air_f [4], c_f [4]) of row i, from the state row, the memory row, the action row and kin's feet"""
    cfg, P, s, m = c.cfg, c.params, c.states[i], c.mem[i]
    nq = cfg.n_joints
    dtc = cfg.sim_dt * cfg.frame_skip
    g = lambda name, k: s[SW[name]:SW[name] + k]
    R0 = ku.quat_to_R(g("quat", 4))
    vb, wb, gb = R0.T @ g("lin_vel", 3), R0.T @ g("ang_vel", 3), R0.T @ np.array([0.0, 0.0, -1.0])
    tau, qd, a = g("tau", nq), g("qd", nq), c.actions[i].astype(np.float64)
    pc, valid = (int(x[i]) for x in mem_ints(c.mem))
    cmask = int(contact_masks(c.states)[i])
    pf = ku.member(kin, "prim_point")[i][list(FOOT_PRIMS)]
    uf = ku.member(kin, "prim_vel")[i][list(FOOT_PRIMS)]
    Ff = ku.member(kin, "prim_force")[i][list(FOOT_PRIMS)]
    cf = np.array([(cmask >> p) & 1 for p in FOOT_PRIMS])
    sp2 = uf[:, 0] ** 2 + uf[:, 1] ** 2
    air = m[MW["air_time"]:MW["air_time"] + 4] + dtc
    first = np.array([bool(valid and cf[f] and not (pc >> f) & 1) for f in range(4)])
    nprims = 24 if nq == 12 else 20
    t = np.zeros(SHAPE_TERMS)
    t[0] = vb[2] ** 2
    t[1] = wb[0] ** 2 + wb[1] ** 2
    t[2] = gb[0] ** 2 + gb[1] ** 2
    t[3] = (s[SW["pos"] + 2] - P.base_height_target) ** 2
    t[4] = (tau ** 2).sum()
    t[5] = (qd ** 2).sum()
    t[6] = (((qd - m[MW["prev_qd"]:MW["prev_qd"] + nq]) / dtc) ** 2).sum() if valid else 0.0
    t[7] = ((a - m[MW["prev_action"]:MW["prev_action"] + nq]) ** 2).sum() if valid else 0.0
    t[8] = np.abs(tau * qd).sum()
    t[9] = np.where(cf == 1, sp2, 0.0).sum()
    t[10] = np.where(cf == 1, 0.0, (pf[:, 2] - P.foot_clearance_target) ** 2 * np.sqrt(sp2)).sum()
    t[11] = np.maximum(0.0, Ff - P.foot_force_max).sum()
    t[12] = np.where(first, air - P.air_time_target, 0.0).sum()
    t[13] = sum((cmask >> p) & 1 for p in range(nprims) if p not in FOOT_PRIMS)
    t[14] = np.exp(-((vb[0] - P.cmd_lin_vel[0]) ** 2 + (vb[1] - P.cmd_lin_vel[1]) ** 2) / P.tracking_sigma)
    t[15] = np.exp(-(wb[2] - P.cmd_yaw_rate) ** 2 / P.tracking_sigma)
    return t, first, air, cf


def reference(c, flags=F_ALL, mask=None):
    """What the call must leave in (mem, reward, terms, ep) for case c, and (first_f [n, 4]) for the coverage assertion.  The reward
    is f32(f64(reward_in) + sum_k w_k term_k) of the REFERENCE's terms (a check compares with the output's own terms, to one ulp)."""
    kin = kin_rows(c)
    mem, reward, terms, ep = c.mem.copy(), c.reward.copy(), c.terms.copy(), c.ep.copy()
    w = np.array(list(c.params.weight))
    nq = c.cfg.n_joints
    firsts = np.zeros((c.n, 4), bool)
    for i in range(c.n):
        if mask is not None and not mask[i]:
            continue
        pc, valid = mem_ints(mem)
        if (flags & F_DONE) and c.done[i]:
            if flags & F_TERMS:
                terms[i] = 0.0
            if flags & F_EP:
                ep[0, i] += 1.0
                ep[1:, i] += mem[i, MW["ep_sum"]:MW["ep_sum"] + SHAPE_TERMS]
            mem[i, MW["ep_sum"]:MW["ep_sum"] + SHAPE_TERMS] = 0.0
            mem[i, MW["air_time"]:MW["air_time"] + 4] = 0.0
            pc[i] = 0; valid[i] = 0
            continue
        t, first, air, cf = reference_terms(c, i, kin)
        firsts[i] = first
        if flags & F_TERMS:
            terms[i] = t
        s = 0.0
        for k in range(SHAPE_TERMS):
            s += w[k] * t[k]
        if flags & F_REWARD:
            reward[i] = np.float32(np.float64(reward[i]) + s)
        mem[i, MW["ep_sum"]:MW["ep_sum"] + SHAPE_TERMS] += w * t
        mem[i, MW["prev_action"]:MW["prev_action"] + nq] = c.actions[i].astype(np.float64)
        mem[i, MW["prev_qd"]:MW["prev_qd"] + nq] = c.states[i, SW["qd"]:SW["qd"] + nq]
        mem[i, MW["air_time"]:MW["air_time"] + 4] = np.where(cf == 1, 0.0, air)
        pc[i] = int(sum(int(cf[f]) << f for f in range(4))); valid[i] = 1
    return (mem, reward, terms, ep), firsts


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_outputs(c, got, want, flags=F_ALL, mask=None):
    """got against want (both (mem, reward, terms, ep)): doubles to kin_util.TOL, the integer members exactly, the reward to one f32
    ulp of f32(f64(reward_in) + sum_k w_k terms_out_k) with the OUTPUT's own terms (the reference's where terms_out is not asked
    for); done rows and masked rows bit for bit (they hold no arithmetic but the sums handed to ep_out)."""
    (gm, gr, gt, ge), (wm, wr, wt, we) = got, want
    live = np.ones(c.n, bool) if mask is None else np.asarray(mask, bool)
    dn = (c.done != 0) & bool(flags & F_DONE)
    calc = live & ~dn
    bad = ~ku.close(gm[live, :MW["prev_contact"]], wm[live, :MW["prev_contact"]], ku.TOL)
    assert not bad.any(), (np.argwhere(bad)[:5], "mem")
    for g, w_ in zip(mem_ints(gm), mem_ints(wm)):
        assert (g == w_).all(), "integer members of mem"
    assert ku.close(gt[live], wt[live], ku.TOL).all(), ("terms", np.abs(gt[live] - wt[live]).max())
    assert ku.close(ge[:, live], we[:, live], ku.TOL).all(), ("ep", np.abs(ge[:, live] - we[:, live]).max())
    w = np.array(list(c.params.weight))
    for i in np.nonzero(calc)[0]:
        if flags & F_REWARD:
            s = 0.0
            for k in range(SHAPE_TERMS):
                s += w[k] * gt[i, k]
            ref = np.float32(np.float64(c.reward[i]) + s) if flags & F_TERMS else wr[i]
            assert abs(np.float64(gr[i]) - np.float64(ref)) <= np.float64(np.spacing(np.abs(ref))), (i, gr[i], ref)
    # rows with no arithmetic of their own: bit for bit
    keep = ~calc
    assert (bits(gr)[np.repeat(keep, 4)] == bits(wr)[np.repeat(keep, 4)]).all(), "reward of done / masked rows"
    assert (bits(gt).reshape(c.n, -1)[keep] == bits(wt).reshape(c.n, -1)[keep]).all(), "terms of done / masked rows"
    assert (bits(gm).reshape(c.n, -1)[keep] == bits(wm).reshape(c.n, -1)[keep]).all(), "mem of done / masked rows"
    assert (bits(ge).reshape(EP_FIELDS, c.n, 8)[:, ~live] == bits(we).reshape(EP_FIELDS, c.n, 8)[:, ~live]).all(), "ep of masked rows"
    assert (bits(ge).reshape(EP_FIELDS, c.n, 8)[:, calc] == bits(we).reshape(EP_FIELDS, c.n, 8)[:, calc]).all(), "ep of rows that did not finish"
    if not (flags & F_REWARD):
        assert (bits(gr) == bits(c.reward)).all()
    if not (flags & F_TERMS):
        assert (bits(gt) == bits(c.terms)).all()
    if not (flags & F_EP):
        assert (bits(ge) == bits(c.ep)).all()
