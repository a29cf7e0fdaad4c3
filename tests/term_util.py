"""What solorl_terminate must give (include/solorl.h, "Early termination"), restated in numpy: fp64 with the same roundings -- numpy
rounds every product, sum and quotient on its own -- and float32 sums where the arrays are float32; the crafted rows the host and the
GPU tests share; and the helper that builds and runs tests/host/terminate_main.cpp (solorl_amd/csrc/termination.hpp compiled alone
by g++)."""
import ctypes as C

import numpy as np

from solorl_amd._native import Termination
from solorl_amd.config import EnvState
from tests.host_util import hex32, hex64, run_host

ROW_WORDS = C.sizeof(EnvState) // 8
HEIGHT, TILT, CONTACT, JOINT = 1, 2, 4, 8
ALL = HEIGHT | TILT | CONTACT | JOINT
EP_FIELDS, STAT_FIELDS = 10, 5
DBL_MAX = np.finfo(np.float64).max
POISON8, POISON32 = 0xAA, 0xAAAAAAAA


def W(member):
    """8-byte word of a member of solorl_env_state"""
    return getattr(EnvState, member).offset // 8


class Params:
    """solorl_termination with plain members"""

    def __init__(self, rules=ALL, min_steps=0, contact_prims=0, min_height=0.0, min_up_z=0.0, contact_force_min=0.0, joint_lo=None, joint_hi=None,
                 terminal_reward=-10.0):
        self.rules, self.min_steps, self.contact_prims = int(rules), int(min_steps), int(contact_prims)
        self.min_height, self.min_up_z, self.contact_force_min = float(min_height), float(min_up_z), float(contact_force_min)
        self.joint_lo = [0.0] * 12 if joint_lo is None else [float(v) for v in joint_lo]
        self.joint_hi = [0.0] * 12 if joint_hi is None else [float(v) for v in joint_hi]
        self.terminal_reward = float(terminal_reward)

    def struct(self):
        p = Termination()
        p.rules, p.min_steps, p.contact_prims = self.rules, self.min_steps, self.contact_prims
        p.min_height, p.min_up_z, p.contact_force_min, p.terminal_reward = self.min_height, self.min_up_z, self.contact_force_min, self.terminal_reward
        for j in range(12):
            p.joint_lo[j], p.joint_hi[j] = self.joint_lo[j], self.joint_hi[j]
        return p

    def but(self, **kw):
        q = Params(self.rules, self.min_steps, self.contact_prims, self.min_height, self.min_up_z, self.contact_force_min, self.joint_lo, self.joint_hi,
                   self.terminal_reward)
        for k, v in kw.items():
            assert hasattr(q, k), k
            setattr(q, k, v)
        return q


def finite(x):
    return bool(x >= -DBL_MAX and x <= DBL_MAX)


def ints(rows, member):
    """the int32 member of every row ([n, 255] float64)"""
    return np.ascontiguousarray(rows).view(np.int32)[:, getattr(EnvState, member).offset // 4]


def fired_bits(robot12, p, sim_dt, row):
    """the rule bits that fire on one row ([255] float64), by the header's table"""
    nq, nprims = (12, 24) if robot12 else (8, 20)
    row = np.asarray(row, dtype=np.float64)
    i32 = row.view(np.int32)
    if int(i32[EnvState.timestep.offset // 4]) < p.min_steps:
        return 0
    out = 0
    with np.errstate(all="ignore"):
        if p.rules & HEIGHT:
            z = row[W("pos") + 2]
            if finite(z) and z < np.float64(p.min_height):
                out |= HEIGHT
        if p.rules & TILT:
            qx, qy = row[W("quat")], row[W("quat") + 1]
            up_z = np.float64(1.0) - np.float64(2.0) * (qx * qx + qy * qy)
            if finite(up_z) and up_z < np.float64(p.min_up_z):
                out |= TILT
        if p.rules & CONTACT:
            bits = p.contact_prims & (int(i32[EnvState.contact_mask.offset // 4]) & 0xFFFFFFFF) & ((1 << nprims) - 1)
            for q in range(nprims):
                if (bits >> q) & 1:
                    f = row[W("lambda_prev") + q] / np.float64(sim_dt)
                    if finite(f) and f >= np.float64(p.contact_force_min):
                        out |= CONTACT
        if p.rules & JOINT:
            for j in range(nq):
                q = row[W("q") + j]
                if finite(q) and (q < np.float64(p.joint_lo[j]) or q > np.float64(p.joint_hi[j])):
                    out |= JOINT
    return out


class Arrays:
    """the arrays a call reads and writes: done, reward, fired (n), timeout, success, ep_reward (n), ep_stats [10, n], stats [5, n]"""
    NAMES = ("done", "reward", "fired", "timeout", "success", "ep_reward", "ep_stats", "stats")

    def __init__(self, n, done, reward, seed=0):
        g = np.random.default_rng(seed)
        self.done = np.asarray(done, dtype=np.uint8).copy()
        self.reward = np.asarray(reward, dtype=np.float32).copy()
        self.fired = np.full(n, POISON8, dtype=np.uint8)
        self.timeout, self.success = np.full(n, POISON8, dtype=np.uint8), np.full(n, POISON8, dtype=np.uint8)
        self.ep_reward = np.full(n, POISON32, dtype=np.uint32).view(np.float32)
        # sums that already hold something (every addition must round as a float32 addition does), a -0.0 among them
        self.ep_stats = g.uniform(-50.0, 50.0, (EP_FIELDS, n)).astype(np.float32)
        self.ep_stats[3, ::2] = -0.0
        self.stats = g.integers(0, 9, (STAT_FIELDS, n)).astype(np.float32)

    def copy(self):
        o = object.__new__(Arrays)
        for k in self.NAMES:
            setattr(o, k, getattr(self, k).copy())
        return o

    def bits(self):
        """name -> the array as unsigned integers, for bitwise comparisons"""
        return {k: (getattr(self, k) if getattr(self, k).dtype == np.uint8 else getattr(self, k).view(np.uint32)) for k in self.NAMES}


def reference(robot12, p, sim_dt, rows, arrays, mask=None, info=True, stats=True):
    """the table of the header on a copy of ``arrays`` -> the copy"""
    a = arrays.copy()
    n = rows.shape[0]
    r = np.float32(p.terminal_reward)
    ts, dr0 = ints(rows, "timestep"), W("dr")
    with np.errstate(all="ignore"):
        for i in range(n):
            if mask is not None and not mask[i]:
                continue
            if a.done[i] != 0:
                a.fired[i] = 0
                continue
            f = fired_bits(robot12, p, sim_dt, rows[i])
            a.fired[i] = f
            if f == 0:
                continue
            a.done[i] = 1
            a.reward[i] = r
            if info:
                a.timeout[i] = a.success[i] = 0
                a.ep_reward[i] = r
                s = a.ep_stats[:, i]
                s[0] = s[0] + np.float32(1.0)
                s[1] = s[1] + r
                s[2] = s[2] + np.float32(ts[i])
                s[3] = s[3] + np.float32(0.0)
                for k in range(5):
                    s[4 + k] = s[4 + k] + np.float32(rows[i, dr0 + k])
            if stats:
                a.stats[0, i] = a.stats[0, i] + np.float32(1.0)
                for k in range(4):
                    if (f >> k) & 1:
                        a.stats[1 + k, i] = a.stats[1 + k, i] + np.float32(1.0)
    return a


# ---- the crafted rows
SIM_DT = 1.0 / 240.0
LO, HI = -1.5, 1.25


def _force_edge(fmin, sim_dt):
    """the smallest impulse whose quotient by sim_dt reaches fmin"""
    lam = np.float64(fmin) * np.float64(sim_dt)
    while lam / np.float64(sim_dt) >= fmin:
        lam = np.nextafter(lam, -np.inf)
    while lam / np.float64(sim_dt) < fmin:
        lam = np.nextafter(lam, np.inf)
    return float(lam)


def params(robot12, **kw):
    """all four rules: height 0.05, tilt up_z < 0.5 (60 degrees, a threshold the arithmetic reaches exactly), base and knee contacts of
    at least 5 N, joint limits [-1.5, 1.25]"""
    nq = 12 if robot12 else 8
    prims = sum(1 << q for q in list(range(12)) + [12, 14, 16, 18])
    p = Params(ALL, 3, prims, 0.05, 0.5, 5.0, [LO] * nq + [0.0] * (12 - nq), [HI] * nq + [0.0] * (12 - nq), -10.0)
    return p.but(**kw) if kw else p


def base_row(timestep=10):
    """a robot standing: no rule of params() fires"""
    row = np.zeros(ROW_WORDS, dtype=np.float64)
    row[W("pos"):W("pos") + 3] = (0.3, -0.2, 0.24)
    row[W("quat"):W("quat") + 4] = (0.0, 0.0, 0.0, 1.0)
    row[W("q"):W("q") + 12] = np.linspace(-0.4, 0.4, 12)
    row[W("dr"):W("dr") + 5] = (1.25, -0.375, -0.0625, 0.5, 3.0)
    i32 = row.view(np.int32)
    i32[EnvState.timestep.offset // 4] = timestep
    i32[EnvState.rng_counter.offset // 4] = 77
    for q in (13, 15, 17, 19):                          # the feet stand on the ground: not in contact_prims
        i32[EnvState.contact_mask.offset // 4] |= 1 << q
        row[W("lambda_prev") + q] = 0.025
    return row


def cases(robot12):
    """[(name, row, done on entry, the bits expected to fire or None = whatever the table says)] with params(robot12)"""
    nq = 12 if robot12 else 8
    out = []

    def add(name, expect=None, done=0, timestep=10, **words):
        row = base_row(timestep)
        i32 = row.view(np.int32)
        for k, v in words.items():
            if k == "cmask":
                i32[EnvState.contact_mask.offset // 4] |= v
            else:
                member, idx = k.rsplit("_", 1)
                row[W(member) + int(idx)] = v
        out.append((name, row, done, expect))

    below, above = (lambda x: float(np.nextafter(np.float64(x), -np.inf))), (lambda x: float(np.nextafter(np.float64(x), np.inf)))
    add("standing", 0)
    # each rule just below, at and just above its threshold
    add("height below", HEIGHT, pos_2=below(0.05)); add("height at", 0, pos_2=0.05); add("height above", 0, pos_2=above(0.05))
    add("tilt past", TILT, quat_0=above(0.5)); add("tilt at", 0, quat_0=0.5); add("tilt short", 0, quat_0=below(0.5))
    add("tilt past y", TILT, quat_1=-above(0.5)); add("tilt both", TILT, quat_0=0.4, quat_1=0.4); add("inverted", TILT, quat_0=1.0)
    edge = _force_edge(5.0, SIM_DT)
    for q in (0, 11, 12, 18):
        add("contact %d at" % q, CONTACT, cmask=1 << q, **{"lambda_prev_%d" % q: edge})
        add("contact %d below" % q, 0, cmask=1 << q, **{"lambda_prev_%d" % q: below(edge)})
        add("contact %d above" % q, CONTACT, cmask=1 << q, **{"lambda_prev_%d" % q: above(edge)})
    add("contact force without the bit", 0, lambda_prev_3=1.0)
    add("contact of a primitive that is not chosen", 0, cmask=1 << 13, lambda_prev_13=1.0)
    add("contact of a shoulder that is not chosen", 0, cmask=1 << 21, lambda_prev_21=1.0)
    add("two contacts, one strong", CONTACT, cmask=(1 << 2) | (1 << 14), lambda_prev_2=below(edge), lambda_prev_14=1.0)
    for j in (0, nq - 1):
        add("joint %d under" % j, JOINT, **{"q_%d" % j: below(LO)}); add("joint %d at lo" % j, 0, **{"q_%d" % j: LO})
        add("joint %d over" % j, JOINT, **{"q_%d" % j: above(HI)}); add("joint %d at hi" % j, 0, **{"q_%d" % j: HI})
    if not robot12:                                    # joints 8..11 of a Solo8 row are not joints
        add("joint 8 of a Solo8", 0, q_8=9.0); add("joint 11 of a Solo8", 0, q_11=-9.0)
    # several rules at once
    add("height and tilt", HEIGHT | TILT, pos_2=0.01, quat_0=0.9)
    add("all four", ALL, pos_2=-0.5, quat_1=0.8, cmask=1 << 5, lambda_prev_5=0.5, q_3=2.0)
    add("contact and joint", CONTACT | JOINT, cmask=1 << 16, lambda_prev_16=0.25, q_1=-3.0)
    # min_steps = 3
    add("fallen at timestep 2", 0, timestep=2, pos_2=0.01, quat_0=0.9)
    add("fallen at timestep 3", HEIGHT | TILT, timestep=3, pos_2=0.01, quat_0=0.9)
    add("fallen at timestep 0", 0, timestep=0, pos_2=0.01)
    # done on entry: the row is the new episode's
    add("done on entry, standing", 0, done=1); add("done on entry, fallen", 0, done=1, pos_2=0.01, quat_0=0.9)
    add("done byte 255 on entry", 0, done=255, pos_2=0.01)
    # non-finite members fire nothing
    for name, v in (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf"))):
        add("pos.z " + name, 0, pos_2=v); add("qx " + name, 0, quat_0=v); add("qy " + name, 0, quat_1=v)
        add("q0 " + name, 0, q_0=v); add("q last " + name, 0, **{"q_%d" % (nq - 1): v})
        add("lambda " + name, 0, cmask=1 << 4, lambda_prev_4=v)
        add("dr " + name + " on a row that does not fire", 0, dr_2=v)
        add("pos.z " + name + " beside a joint over", JOINT, pos_2=v, q_2=2.0)
    add("qx huge: up_z overflows", 0, quat_0=1e200)
    add("lambda huge: the force overflows", 0, cmask=1 << 4, lambda_prev_4=1e307)
    add("dr +inf on a row that fires", HEIGHT, pos_2=0.0, dr_4=float("inf"))
    add("members that are not read", 0, pos_0=float("nan"), quat_2=float("nan"), quat_3=float("inf"), treadmill_y_0=float("nan"))
    return out


def batch(robot12, n, seed=1):
    """n rows cycling through cases(robot12) (n < the number of cases: the first n) -> (rows [n, 255], done [n], reward [n], names)"""
    cs = cases(robot12)
    g = np.random.default_rng(seed)
    rows = np.stack([cs[i % len(cs)][1] for i in range(n)])
    done = np.array([cs[i % len(cs)][2] for i in range(n)], dtype=np.uint8)
    reward = g.uniform(-1.0, 1.0, n).astype(np.float32)
    return rows, done, reward, [cs[i % len(cs)][0] for i in range(n)]


# ---- the host program (tests/host/terminate_main.cpp: host_util.build_host("terminate_main"))
def host_terminate(exe, robot12, p, sim_dt, rows, arrays, mask=None, info=True, stats=True, check=False):
    """one call of the host program on ``arrays`` -> the arrays after it (a new Arrays; members the call was not given stay as they
    were), or None if ``check`` and the parameters are refused"""
    n = rows.shape[0]
    hx64, hx32 = hex64, hex32
    dec = lambda v: " ".join(str(int(b)) for b in v)
    text = ["%d %d %s %d %d %d %d" % (1 if robot12 else 0, n, hx64([sim_dt]), int(check), int(mask is not None), int(info), int(stats)),
            "%d %d %d %s" % (p.rules, p.min_steps, p.contact_prims,
                             hx64([p.min_height, p.min_up_z, p.contact_force_min] + p.joint_lo + p.joint_hi + [p.terminal_reward]))]
    if mask is not None:
        text.append(dec(np.asarray(mask, dtype=np.uint8)))
    text += [dec(arrays.done), hx32(arrays.reward), dec(arrays.fired)]
    if info:
        text += [dec(arrays.timeout), dec(arrays.success), hx32(arrays.ep_reward), hx32(arrays.ep_stats)]
    if stats:
        text.append(hx32(arrays.stats))
    text += [hx64(rows[i]) for i in range(n)]
    lines = run_host(exe, input="\n".join(text) + "\n").strip().split("\n")
    if lines[0] == "refused":
        return None
    out = arrays.copy()
    names = ["done", "reward", "fired"] + (["timeout", "success", "ep_reward", "ep_stats"] if info else []) + (["stats"] if stats else [])
    assert len(lines) == len(names), (len(lines), names)
    for name, line in zip(names, lines):
        cur = getattr(out, name)
        if cur.dtype == np.uint8:
            setattr(out, name, np.array([int(x) for x in line.split()], dtype=np.uint8).reshape(cur.shape))
        else:
            setattr(out, name, np.array([int(x, 16) for x in line.split()], dtype=np.uint32).view(np.float32).reshape(cur.shape))
    return out


def same(a, b):
    """the names of the arrays whose bits differ"""
    x, y = a.bits(), b.bits()
    return [k for k in Arrays.NAMES if not np.array_equal(x[k], y[k])]
