"""Shared by tests/test_dyn_host.py and tests/test_dyn_gpu.py: the stand-alone host program (tests/host/rows_main.cpp) and the
comparisons the rows of solorl_dynamics are held to (check_rows) -- the oracle's dense mass matrix, bias and forward dynamics, the
rows of solorl_kinematics for the same states, and a restatement of the foot Jacobians and their Jdot v written here in numpy from
solorl_amd/models/*.json and tests/kin_util.fk (nothing of the engine's source).  Inputs: tests/kin_util.inputs."""
import functools

import numpy as np

from solorl_amd.dyn_tensors import MEMBERS, ROW_WORDS, NV
from tests import kin_util as ku
from tests.util import clone

TOL = ku.TOL            # 1e-10 max(1, |ref|): both sides fp64, short chains
TOL_FD = ku.TOL_FD      # central differences of the oracle's potential energy, h = 1e-6 (measured on the oracle alone: 2e-8)
TOL_M = 1e-10           # |M_ab - ref_ab| <= TOL_M sqrt(ref_aa ref_bb): the scale of an SPD matrix whose diagonal runs from 5e-4 to 2.5
TOL_FWD = 1e-6          # forward dynamics, relative to max |ref|: cond(M) 1.1e4 .. 1.4e4 times the 1e-10 allowed on the entries
ACC_H = 1e-4            # second central difference of the material point's position, on velocities scaled by 0.1
TOL_ACC = 3e-6          # ten times what the numpy recursion measures against that difference (2.8e-7 Solo12, 1.5e-7 Solo8)
TAU_SEED = 777
FOOT_PRIMS = (13, 15, 17, 19)
PERM = np.array([3, 4, 5, 0, 1, 2] + list(range(6, NV)))      # ours [lin, ang, joints] <- the oracle's [ang, lin, joints]

# the host program (tests/kin_util.rows_main) asked for the rows of solorl_dynamics, and a member's view of them
dyn_main = ku.rows_main
run_dyn_main = functools.partial(ku.run_rows_main, "dyn", ROW_WORDS)
member = functools.partial(ku.rows_member, MEMBERS)


def no_damping(cfg):
    c = cfg.copy()
    c.damping = 0.0
    return c


def velocity(s):
    return np.array(list(s.lin_vel) + list(s.ang_vel) + list(s.qd))


def scaled_m_close(M, ref, tol=TOL_M):
    d = np.sqrt(np.diag(ref))
    return np.abs(M - ref) <= tol * np.outer(d, d)


def leg_of_column(robot):
    """generalised coordinate 6 + j -> leg of joint j (the root of its chain under the base)"""
    md = ku.model(robot)
    roots = sorted(i for i, L in enumerate(md["links"]) if i > 0 and L["parent"] == 0)
    out = {}
    for j, i in enumerate(md["dof_links"]):
        while md["links"][i]["parent"] != 0:
            i = md["links"][i]["parent"]
        out[6 + j] = roots.index(i)
    return out


# ---------------------------------------------------------------- numpy restatement: foot Jacobian and Jdot v
def foot_jac_acc(robot, s, P, scale=1.0):
    """Jacobian [4,3,NV] and Jdot v [4,3] of the material points of the feet's links at the world points P [4,3], for state s with all
    velocities multiplied by `scale`: columns e_k, e_k x (P - pos), a_j x (P - o_j) on the leg's own joints; Jdot v from the recursion
    of the links' bias accelerations (all generalised accelerations zero)."""
    md = ku.model(robot)
    nl = md["nlinks"]
    R, o, _ = ku.fk_state(robot, s)
    pos = np.array(s.pos)
    qd = np.array(s.qd) * scale
    w, alb, aob, a = np.zeros((nl, 3)), np.zeros((nl, 3)), np.zeros((nl, 3)), np.zeros((nl, 3))
    w[0] = np.array(s.ang_vel) * scale
    for i, L in enumerate(md["links"]):
        if i == 0:
            continue
        p = L["parent"]
        r = o[i] - o[p]
        a[i] = R[p] @ np.array(L["axis"], float)
        qdi = qd[md["dof_links"].index(i)] if L["jtype"] == 0 else 0.0
        w[i] = w[p] + qdi * a[i]
        alb[i] = alb[p] + qdi * np.cross(w[p], a[i])
        aob[i] = aob[p] + np.cross(alb[p], r) + np.cross(w[p], np.cross(w[p], r))
    J, acc = np.zeros((4, 3, NV)), np.zeros((4, 3))
    for leg, prim in enumerate(FOOT_PRIMS):
        l = md["prims"][prim]["link"]
        J[leg, :, 0:3] = np.eye(3)
        for k in range(3):
            J[leg, :, 3 + k] = np.cross(np.eye(3)[k], P[leg] - pos)
        i = l
        while i > 0:
            if md["links"][i]["jtype"] == 0:
                J[leg, :, 6 + md["dof_links"].index(i)] = np.cross(a[i], P[leg] - o[i])
            i = md["links"][i]["parent"]
        rp = P[leg] - o[l]
        acc[leg] = aob[l] + np.cross(alb[l], rp) + np.cross(w[l], np.cross(w[l], rp))
    return J, acc


def foot_acc_by_differences(robot, s, P, scale, h=ACC_H):
    """second central difference of the feet's material points along the state's own (scaled) velocities"""
    md = ku.model(robot)
    t = clone(s)
    for k in range(3):
        t.lin_vel[k] *= scale; t.ang_vel[k] *= scale
    for j in range(12):
        t.qd[j] *= scale
    R, o, _ = ku.fk_state(robot, t)
    Rp, op, _ = ku.fk_state(robot, t, h)
    Rm, om, _ = ku.fk_state(robot, t, -h)
    acc = np.zeros((4, 3))
    for leg, prim in enumerate(FOOT_PRIMS):
        l = md["prims"][prim]["link"]
        loc = R[l].T @ (P[leg] - o[l])
        acc[leg] = ((op[l] + Rp[l] @ loc) - 2 * (o[l] + R[l] @ loc) + (om[l] + Rm[l] @ loc)) / (h * h)
    return acc


# ---------------------------------------------------------------- the comparisons
def check_rows(robot, cfg, states, rows, kin_rows, restatement=True):
    """The five comparisons of the issue on rows [n, ROW_WORDS] computed from `states` under `cfg` (its damping included), with
    kin_rows = the rows of solorl_kinematics for the same states from the same kind of producer.  Every sample, every member.
    restatement=False leaves out the check of the numpy restatement against differences (it does not depend on the rows)."""
    from oracle.oracle_py import Oracle
    md = ku.model(robot)
    nq = cfg.n_joints
    nv = 6 + nq
    perm = PERM[:nv]
    orc = Oracle(cfg, 1)
    mass = sum(L["mass"] for L in md["links"])
    legcol = leg_of_column(robot)
    rng = np.random.default_rng(TAU_SEED)
    g = lambda name: member(rows, name)
    kg = lambda name: ku.member(kin_rows, name)
    worst = {}

    def hold(ok, what, i, err=None):
        assert np.all(ok), (what, i, err)

    for i, s in enumerate(states):
        M, bias, grav = g("mass_matrix")[i], g("bias")[i], g("gravity")[i]
        J, jdv, fpos = g("foot_jac")[i], g("foot_acc_bias")[i], g("foot_pos")[i]
        v = velocity(s)
        # 1. the mass matrix
        orc.set_state(0, s)
        Mo, ho = orc.mass_matrix(0)
        Mref, href = Mo[np.ix_(perm, perm)], ho[perm]
        hold(scaled_m_close(M[:nv, :nv], Mref), "mass_matrix", i, np.abs(M[:nv, :nv] - Mref).max())
        assert (M.view(np.int64) == M.T.view(np.int64)).all(), ("M == M^T bit for bit", i)
        for a in range(6, nv):
            for b in range(6, nv):
                if legcol[a] != legcol[b]:
                    assert M[a, b].tobytes() == np.float64(0.0).tobytes(), ("leg-to-other-leg block reads +0.0", i, a, b)
        for name, arr in (("mass_matrix", M[nv:]), ("mass_matrix", M[:, nv:]), ("bias", bias[nv:]), ("gravity", grav[nv:]), ("foot_jac", J[:, :, nv:])):
            assert (arr.view(np.int64) == 0).all(), ("padding reads 0", name, i)
        np.linalg.cholesky(M[:nv, :nv])
        # 2. bias and gravity
        hold(ku.close(bias[:nv], href, TOL), "bias", i, np.abs(bias[:nv] - href).max())
        rest = clone(s)
        for k in range(3):
            rest.lin_vel[k] = 0.0; rest.ang_vel[k] = 0.0
        for j in range(12):
            rest.qd[j] = 0.0
        orc.set_state(0, rest)
        hold(ku.close(grav[:nv], orc.mass_matrix(0)[1][perm], TOL), "gravity", i)
        hold(ku.close(grav[0:3], [0.0, 0.0, mass * cfg.gravity], TOL), "gravity[0:3]", i)
        dV = np.zeros(nq)
        for j in range(nq):
            for sgn in (1, -1):
                t = clone(rest)
                t.q[j] += sgn * ku.FD_H
                orc.set_state(0, t)
                dV[j] += sgn * orc.energy_momentum(0)["V"] / (2 * ku.FD_H)
        hold(ku.close(grav[6:nv], dV, TOL_FD), "gravity[6:] = dV/dq", i, np.abs(grav[6:nv] - dV).max())
        # 3. against the kinematics rows of the same states
        Mv = M @ v
        lin_mom, ang_mom = kg("lin_mom")[i], kg("ang_mom")[i]
        hold(ku.close(0.5 * v @ Mv, kg("kinetic")[i], TOL), "kinetic", i)
        hold(ku.close(Mv[0:3], lin_mom, TOL), "lin_mom", i)
        hold(ku.close(Mv[3:6], ang_mom - np.cross(np.array(s.pos), lin_mom), TOL), "ang_mom about pos", i)
        for leg, prim in enumerate(FOOT_PRIMS):
            hold(ku.close(J[leg] @ v, kg("prim_vel")[i][prim], TOL), "foot_jac v = prim_vel", i)
            hold(ku.close(fpos[leg], kg("prim_point")[i][prim], TOL), "foot_pos = prim_point", i)
        # 4. the numpy restatement
        P = kg("prim_point")[i][list(FOOT_PRIMS)]
        Jn, an = foot_jac_acc(robot, s, P)
        hold(ku.close(J, Jn, TOL), "foot_jac", i, np.abs(J - Jn).max())
        hold(ku.close(jdv, an, TOL), "foot_acc_bias", i, np.abs(jdv - an).max())
        for leg in range(4):
            for c in range(6, NV):
                if legcol.get(c, -1) != leg:
                    assert not J[leg, :, c].any(), ("columns of other legs read 0", i, leg, c)
        if restatement:
            _, a01 = foot_jac_acc(robot, s, P, scale=0.1)
            fd = foot_acc_by_differences(robot, s, P, 0.1)
            err = np.abs(a01 - fd) / np.maximum(1.0, np.abs(fd))
            worst["restatement"] = max(worst.get("restatement", 0.0), err.max())
            hold(err <= TOL_ACC, "numpy Jdot v against second differences", i, err.max())
        # 5. forward dynamics
        tau = rng.uniform(-3, 3, nq)
        t = clone(s)
        for j in range(nq):
            t.tau[j] = tau[j]
        orc.set_state(0, t)
        ref = orc.forward_dynamics(0)[perm]
        got = np.linalg.solve(M[:nv, :nv], np.concatenate((np.zeros(6), tau)) - bias[:nv])
        hold(np.abs(got - ref) <= TOL_FWD * np.abs(ref).max(), "forward dynamics", i, np.abs(got - ref).max() / np.abs(ref).max())
    return worst
