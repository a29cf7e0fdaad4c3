"""Shared by tests/test_kin_host.py and tests/test_kin_gpu.py: the seeded inputs of the solorl_kinematics checks, the stand-alone host
program (tests/host/rows_main.cpp, which tests/dyn_util.py runs too) and the three references its rows are compared with -- the oracle's prim_points and
energy_momentum, and a forward kinematics written here in numpy from solorl_amd/models/*.json (nothing of the engine's source)."""
import ctypes as C
import functools
import json
import os
import tempfile

import numpy as np

from solorl_amd.config import EnvState, SoloConfig, default_config, ROBOT_SOLO12, TASK_WALK
from solorl_amd.kinematics import EnvKin, MEMBERS, ROW_WORDS
from tests.host_util import ROOT, build_host, run_host, san_flags, sanitizers_link

TOL = 1e-10          # |err| <= TOL * max(1, |value|): both sides fp64, a chain of at most 5 frames, ~100 roundings on O(10) magnitudes
TOL_FD = 1e-6        # central differences with h = 1e-6: truncation O(h^2) + rounding 1e-16 / h
FD_H = 1e-6
SEED = 20240611      # no sample of it has two foot rings tied to 1e-12 (test_kin_host.py checks)
CASES = [(robot, urdf) for robot in (0, 1) for urdf in (0, 1)]


def kin_cfg(robot, urdf):
    c = default_config(robot, TASK_WALK)
    c.use_urdf_inertia = urdf
    c.disable_termination = 1
    return c


# ---------------------------------------------------------------- the host program
def host_main(program, sanitize=False):
    """Path of tests/host/<program>.cpp built by g++ (once per process), or None if sanitize is asked for and the sanitizer runtimes do
    not link here."""
    if sanitize and not sanitizers_link():
        return None
    return build_host(program, san_flags(program) if sanitize else ())


rows_main = functools.partial(host_main, "rows_main")


def run_rows_main(query, row_words, cfg, states, sanitize=False):
    """query: "kin" or "dyn"; states: sequence of EnvState -> float64 [n, row_words] of the host program's rows"""
    exe = rows_main(sanitize)
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(bytes(cfg)); f.write(np.array([len(states), 0], np.int32).tobytes())
            for s in states:
                f.write(bytes(s))
        run_host(exe, (query, fin, fout), timeout=120)
        return np.fromfile(fout, np.float64).reshape(len(states), row_words)


def rows_member(members, rows, name):
    """view of member `name` (offset and shape from `members`) in rows [n, row words] (numpy)"""
    off, shape = members[name]
    n = int(np.prod(shape)) if shape else 1
    v = rows[:, off // 8: off // 8 + n]
    return v.reshape((rows.shape[0],) + tuple(shape)) if shape else v[:, 0]


kin_main = rows_main
run_kin_main = functools.partial(run_rows_main, "kin", ROW_WORDS)
member = functools.partial(rows_member, MEMBERS)      # of solorl_env_kin


# ---------------------------------------------------------------- inputs
def random_states(cfg, n, rng):
    """uniform random base orientation, joints in +-3 rad, velocities up to 3 m/s and 30 rad/s; random contact flags and impulses"""
    out = []
    nq = cfg.n_joints
    for _ in range(n):
        s = EnvState()
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        s.pos[:] = list(rng.uniform(-2, 2, 3)); s.quat[:] = list(q)
        s.lin_vel[:] = list(rng.uniform(-3, 3, 3)); s.ang_vel[:] = list(rng.uniform(-30, 30, 3))
        for j in range(nq):
            s.q[j] = rng.uniform(-3, 3); s.qd[j] = rng.uniform(-30, 30)
        for p in range(24):
            s.lambda_prev[p] = rng.uniform(0, 0.05)
        s.contact_mask = int(rng.integers(0, 1 << 24))
        out.append(s)
    return out


def rollout_states(cfg, n, seed):
    """n states of oracle rollouts under random actions, taken while primitives touch the ground"""
    from oracle.oracle_py import Oracle
    rng = np.random.default_rng(seed)
    orc = Oracle(cfg, 4, seed=seed)
    orc.reset()
    out = []
    for t in range(400):
        orc.step(rng.uniform(-1, 1, (4, cfg.n_joints)))
        if t % 3 == 2:
            for i in range(4):
                s = orc.get_state(i)
                if s.contact_mask & 0xFFFFFF and len(out) < n:
                    out.append(s)
        if len(out) >= n:
            break
    assert len(out) == n, len(out)
    return out


_INPUTS = {}


def inputs(robot, urdf):
    """(cfg, 64 states: 32 random poses then 32 rollout states), computed once per process and never modified"""
    if (robot, urdf) not in _INPUTS:
        cfg = kin_cfg(robot, urdf)
        rng = np.random.default_rng(SEED + 10 * robot + urdf)
        _INPUTS[(robot, urdf)] = (cfg, random_states(cfg, 32, rng) + rollout_states(cfg, 32, SEED + 10 * robot + urdf))
    return _INPUTS[(robot, urdf)]


# ---------------------------------------------------------------- numpy forward kinematics from the model JSON
_MODELS = {}


def model(robot):
    if robot not in _MODELS:
        _MODELS[robot] = json.load(open(os.path.join(ROOT, "solorl_amd", "models", "solo12.json" if robot == ROBOT_SOLO12 else "solo8.json")))
    return _MODELS[robot]


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def axis_angle_R(axis, angle):
    a = np.asarray(axis, float)
    th = np.linalg.norm(a) * angle
    if th == 0.0:
        return np.eye(3)
    k = a / np.linalg.norm(a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def fk(robot, pos, R0, q):
    """-> (R [nl,3,3], o [nl,3], c [nl,3]): link axes, frame origins and centres of mass in the world"""
    md = model(robot)
    nl = md["nlinks"]
    R, o, c = np.zeros((nl, 3, 3)), np.zeros((nl, 3)), np.zeros((nl, 3))
    for i, L in enumerate(md["links"]):
        if i == 0:
            R[0], o[0] = R0, pos
        else:
            p = L["parent"]
            o[i] = o[p] + R[p] @ np.array(L["jorigin"])
            R[i] = R[p] @ axis_angle_R(L["axis"], q[md["dof_links"].index(i)]) if L["jtype"] == 0 else R[p]
        c[i] = o[i] + R[i] @ np.array(L["com"])
    return R, o, c


def fk_state(robot, s, h=0.0):
    """forward kinematics of state s moved along its own velocities for a time h (exactly: the base turns by exp(h [w]x))"""
    w = np.array(s.ang_vel)
    R0 = axis_angle_R(w, h) @ quat_to_R(np.array(s.quat)) if h != 0.0 else quat_to_R(np.array(s.quat))
    return fk(robot, np.array(s.pos) + h * np.array(s.lin_vel), R0, np.array(s.q) + h * np.array(s.qd))


def close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


def check_rows(robot, cfg, states, rows, oracle_cfg=None):
    """The three comparisons of the issue on rows [n, ROW_WORDS] computed from `states`: oracle prim_points, oracle
    energy_momentum, numpy forward kinematics (+ central differences for the velocities).  Every sample, every member."""
    from oracle.oracle_py import Oracle
    md = model(robot)
    nl, npr = md["nlinks"], len(md["prims"])
    orc = Oracle(oracle_cfg or cfg, 1)
    mass = sum(L["mass"] for L in md["links"])
    for i, s in enumerate(states):
        g = lambda name: member(rows, name)[i]
        orc.set_state(0, s)
        # 1. support points
        pp = orc.prim_points(0)
        assert close(g("prim_point")[:npr], pp[:npr, :3], TOL).all(), (i, np.abs(g("prim_point")[:npr] - pp[:npr, :3]).max())
        # 2. energy and momentum
        em = orc.energy_momentum(0)
        for name, ref in (("kinetic", em["T"]), ("potential", em["V"]), ("lin_mom", em["p"]), ("ang_mom", em["L"])):
            assert close(g(name), ref, TOL).all(), (i, name, g(name), ref)
        # 3. frames against the numpy forward kinematics
        R, o, c = fk_state(robot, s)
        assert close(g("link_pos")[:nl], o, TOL).all(), (i, "link_pos")
        assert close(g("link_com")[:nl], c, TOL).all(), (i, "link_com")
        lq = g("link_quat")[:nl]
        assert np.allclose(np.linalg.norm(lq, axis=1), 1.0, rtol=0, atol=1e-14) and (lq[:, 3] >= 0).all(), (i, "link_quat unit, w >= 0")
        for l in range(nl):
            assert close(quat_to_R(lq[l]), R[l], TOL).all(), (i, l, "link_quat")
        # velocities: central differences of the same forward kinematics
        Rp, op, cp = fk_state(robot, s, FD_H)
        Rm, om, cm = fk_state(robot, s, -FD_H)
        assert close(g("link_com_vel")[:nl], (cp - cm) / (2 * FD_H), TOL_FD).all(), (i, "link_com_vel")
        for p in range(npr):
            l = md["prims"][p]["link"]
            loc = R[l].T @ (g("prim_point")[p] - o[l])         # the link's material point at the support point
            fd = ((op[l] + Rp[l] @ loc) - (om[l] + Rm[l] @ loc)) / (2 * FD_H)
            assert close(g("prim_vel")[p], fd, TOL_FD).all(), (i, p, "prim_vel", g("prim_vel")[p], fd)
        # angular velocity: the antisymmetric part of dR/dt R^T
        for l in range(nl):
            W = (Rp[l] - Rm[l]) / (2 * FD_H) @ R[l].T
            assert close(g("link_ang_vel")[l], [W[2, 1], W[0, 2], W[1, 0]], TOL_FD).all(), (i, l, "link_ang_vel")
        # totals
        assert close(g("mass"), mass, TOL) and close(g("com"), (np.array([L["mass"] for L in md["links"]])[:, None] * c).sum(0) / mass, TOL).all()
        assert close(g("com_vel") * mass, em["p"], TOL).all()
        # normal forces: lambda_prev / sim_dt under the contact mask, bit for bit
        lam = np.array(s.lambda_prev)
        ref = np.where((s.contact_mask >> np.arange(24)) & 1, lam / cfg.sim_dt, 0.0)
        ref[npr:] = 0.0
        assert (g("prim_force").view(np.int64) == ref.view(np.int64)).all(), (i, "prim_force")
        # what the robot does not have reads 0
        for name in ("link_pos", "link_quat", "link_com", "link_com_vel", "link_ang_vel"):
            assert not g(name)[nl:].any(), (i, name)
        assert not g("prim_point")[npr:].any() and not g("prim_vel")[npr:].any()


def foot_ring_gaps(robot, states):
    """smallest gap between the two best profile rings (r_i s + y_i a) of any foot of any state"""
    md = model(robot)
    gap = np.inf
    for s in states:
        R, _, _ = fk_state(robot, s)
        for pr in md["prims"]:
            if len(pr["ring_r"]) > 1:
                d = -R[pr["link"]].T[:, 2]                  # world down in link axes
                a = abs(d[pr["axis"]])
                sp = np.sqrt(max(d @ d - a * a, 0.0) + 1e-12)
                v = np.sort(np.array(pr["ring_r"]) * sp + np.array(pr["ring_y"]) * a)
                gap = min(gap, v[-1] - v[-2])
    return gap
