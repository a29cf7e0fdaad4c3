"""What solorl_randomize_reset must give (include/solorl.h, "Randomised initial states"), restated in numpy from the draw table with the
oracle's Philox (oracle.oracle_py.philox) and the oracle's support points (oracle_prim_points) -- nothing of the engine's own code; the
crafted rows the host and the GPU tests share; and the helper that builds and runs tests/host/reset_random_main.cpp
(solorl_amd/csrc/reset_random.hpp compiled by g++, no -march=native, contraction off).

Python floats are doubles and every operation below rounds on its own, as the header says the draws do: q, qd, lin_vel, ang_vel, count
and the contact words are compared bit for bit.  quat goes through sin and cos and pos.z through the kinematics: those two are compared
to TOL_TRIG."""
import ctypes as C
import math

import numpy as np

from oracle import oracle_py
from solorl_amd._native import ResetRandomization
from solorl_amd.config import EnvState, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK, default_config
from tests.host_util import bits64 as bits, hex64, philox_block, run_host, u24

ROW_WORDS = C.sizeof(EnvState) // 8
STREAM = 8
HEAD_WORDS = 37
TOL_TRIG = 1e-12      # absolute, on quat (order 1) and pos.z (order 1 m): libm's sin / cos against numpy's differ by ulps, 1e-16
TOL_PLACE = 1e-9      # [m] the lowest support point against the clearance: an fp64 chain of metre-sized terms, 1e-14
POISON = 0xAAAAAAAAAAAAAAAA


def W(member):
    """8-byte word of a member of solorl_env_state"""
    return getattr(EnvState, member).offset // 8


MASK_WORD = W("contact_mask")
# the words a call may write: the head, lambda_prev and the contact_mask word
WRITTEN = np.zeros(ROW_WORDS, bool)
WRITTEN[:HEAD_WORDS] = True
WRITTEN[W("lambda_prev"):W("lambda_prev") + 24] = True
WRITTEN[MASK_WORD] = True
QUAT = slice(W("quat"), W("quat") + 4)
POS_Z = W("pos") + 2
APPROX = np.zeros(ROW_WORDS, bool)      # the words compared to TOL_TRIG; every other word bit for bit
APPROX[QUAT] = True
APPROX[POS_Z] = True


def cfg_of(robot12):
    return default_config(ROBOT_SOLO12 if robot12 else ROBOT_SOLO8, TASK_WALK)


class Params:
    """solorl_reset_randomization with plain members, and the joint_limit of the config that goes with it"""

    def __init__(self, seed=1, id0=0, joint_pos=0.0, joint_vel=0.0, lin_vel=0.0, ang_vel=0.0, yaw=0.0, roll=0.0, pitch=0.0, clearance=0.0,
                 place_on_ground=0, joint_limit=10.0):
        vec = lambda x, n: [float(v) for v in np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))]
        self.seed, self.id0 = int(seed), int(id0)
        self.joint_pos, self.joint_vel, self.lin_vel, self.ang_vel = vec(joint_pos, 12), vec(joint_vel, 12), vec(lin_vel, 3), vec(ang_vel, 3)
        self.yaw, self.roll, self.pitch, self.clearance = float(yaw), float(roll), float(pitch), float(clearance)
        self.place_on_ground, self.joint_limit = int(place_on_ground), float(joint_limit)

    def but(self, **kw):
        q = Params()
        q.__dict__.update({k: (list(v) if isinstance(v, list) else v) for k, v in self.__dict__.items()})
        for k, v in kw.items():
            assert hasattr(q, k), k
            setattr(q, k, v)
        return q

    def struct(self):
        p = ResetRandomization()
        p.seed, p.env_id_offset = self.seed, self.id0
        for j in range(12):
            p.joint_pos[j], p.joint_vel[j] = self.joint_pos[j], self.joint_vel[j]
        for k in range(3):
            p.lin_vel[k], p.ang_vel[k] = self.lin_vel[k], self.ang_vel[k]
        p.yaw, p.roll, p.pitch, p.clearance, p.place_on_ground = self.yaw, self.roll, self.pitch, self.clearance, self.place_on_ground
        return p

    def config(self, robot12):
        c = cfg_of(robot12)
        c.joint_limit = self.joint_limit
        return c

    def doubles(self):
        return self.joint_pos + self.joint_vel + self.lin_vel + self.ang_vel + [self.yaw, self.roll, self.pitch, self.clearance]


def full(robot12, **kw):
    """every half-width non-zero, each joint and axis its own; joint_limit 1 so that the clamp is met"""
    nq = 12 if robot12 else 8
    p = Params(seed=0x1234567887654321, id0=5, joint_pos=[0.2 + 0.01 * j for j in range(12)], joint_vel=[1.0 + 0.1 * j for j in range(12)],
               lin_vel=[0.3, 0.2, 0.1], ang_vel=[0.4, 0.5, 0.6], yaw=math.pi, roll=0.1, pitch=0.15, clearance=0.0, place_on_ground=1, joint_limit=1.0)
    for j in range(nq, 12):
        p.joint_pos[j] = p.joint_vel[j] = 0.0
    return p.but(**kw) if kw else p


# ---------------------------------------------------------------- the reference: the draw table in Python floats
def block(seed, gid, k, b):
    return philox_block(seed, gid, 16 * k + b, STREAM)


def delta(word, a):
    return (2.0 * u24(word) - 1.0) * a


def quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


_ORACLE = {}


def support_z(robot12, row):
    """z of the support points of the robot's collision primitives on one row ([255] float64), by the oracle"""
    if robot12 not in _ORACLE:
        _ORACLE[robot12] = oracle_py.Oracle(cfg_of(robot12), 1)
    orc = _ORACLE[robot12]
    orc.set_state(0, EnvState.from_buffer_copy(np.ascontiguousarray(row).tobytes()))
    return orc.prim_points(0)[:24 if robot12 else 20, 2].copy()


def pose_changes(robot12, p):
    nq = 12 if robot12 else 8
    return any(a != 0.0 for a in p.joint_pos[:nq]) or p.yaw != 0.0 or p.roll != 0.0 or p.pitch != 0.0 or p.place_on_ground != 0


def reference_row(robot12, p, row, k, gid):
    """one live row ([255] float64, finite) of episode k -> the row after the call"""
    nq = 12 if robot12 else 8
    r = np.array(row, dtype=np.float64, copy=True)
    lim = np.float64(p.joint_limit)
    for b in range(3):
        for members, widths in ((W("q"), p.joint_pos), (W("qd"), p.joint_vel)):
            if 4 * b >= nq:
                continue
            words = block(p.seed, gid, k, b + (3 if members == W("qd") else 0))
            for w in range(4):
                j = 4 * b + w
                if widths[j] != 0.0:
                    x = np.float64(float(r[members + j]) + delta(words[w], widths[j]))
                    r[members + j] = x if members == W("qd") else np.fmin(np.fmax(x, -lim), lim)
    b6, b7, b8 = (block(p.seed, gid, k, b) for b in (6, 7, 8))
    for w in range(3):
        if p.lin_vel[w] != 0.0:
            r[W("lin_vel") + w] = float(r[W("lin_vel") + w]) + delta(b6[w], p.lin_vel[w])
        if p.ang_vel[w] != 0.0:
            r[W("ang_vel") + w] = float(r[W("ang_vel") + w]) + delta(b7[w], p.ang_vel[w])
    if p.yaw != 0.0 or p.roll != 0.0 or p.pitch != 0.0:
        psi = delta(b6[3], p.yaw) if p.yaw != 0.0 else 0.0
        phi = delta(b7[3], p.roll) if p.roll != 0.0 else 0.0
        th = delta(b8[0], p.pitch) if p.pitch != 0.0 else 0.0
        q = quat_mul(np.array([0.0, 0.0, math.sin(psi / 2), math.cos(psi / 2)]), r[QUAT])
        q = quat_mul(q, np.array([math.sin(phi / 2), 0.0, 0.0, math.cos(phi / 2)]))
        q = quat_mul(q, np.array([0.0, math.sin(th / 2), 0.0, math.cos(th / 2)]))
        q = q / np.linalg.norm(q)
        r[QUAT] = -q if q[3] < 0 else q
    if p.place_on_ground:
        r[POS_Z] = r[POS_Z] + (p.clearance - support_z(robot12, r).min())
    if pose_changes(robot12, p):
        r[W("lambda_prev"):W("lambda_prev") + 24] = 0.0
        r.view(np.uint32)[2 * MASK_WORD] &= 0xFF000000
    return r


def reference(robot12, p, rows, count, mask=None, live=None):
    """the table on copies of rows [n, 255] and count [n] uint32 -> (rows, count); ``live``: the rows to compute (default: all selected
    ones; a caller leaves rows with non-finite members out)"""
    out, cnt = rows.copy(), count.copy()
    for i in range(rows.shape[0]):
        if mask is not None and not mask[i]:
            continue
        cnt[i] = (int(count[i]) + 1) & 0xFFFFFFFF
        if live is None or live[i]:
            out[i] = reference_row(robot12, p, rows[i], int(count[i]), p.id0 + i)
    return out, cnt


# ---------------------------------------------------------------- rows
def random_rows(robot12, n, seed):
    """n rows: every word poison, then the head members -- a base between 0.3 m below and 0.6 m above the ground, any orientation,
    joints within +-0.9 rad -- random impulses, random contact_mask bits (24.. among them) and counters"""
    g = np.random.default_rng(seed)
    rows = np.full((n, ROW_WORDS), POISON, dtype=np.uint64).view(np.float64)
    q = g.normal(size=(n, 4))
    rows[:, W("pos"):W("pos") + 3] = np.stack([g.uniform(-2, 2, n), g.uniform(-2, 2, n), g.uniform(-0.3, 0.6, n)], axis=1)
    rows[:, QUAT] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rows[:, W("lin_vel"):W("lin_vel") + 3] = g.uniform(-1, 1, (n, 3))
    rows[:, W("ang_vel"):W("ang_vel") + 3] = g.uniform(-3, 3, (n, 3))
    rows[:, W("q"):W("q") + 12] = g.uniform(-0.9, 0.9, (n, 12))
    rows[:, W("qd"):W("qd") + 12] = g.uniform(-10, 10, (n, 12))
    rows[:, W("lambda_prev"):W("lambda_prev") + 24] = g.uniform(0, 0.05, (n, 24))
    i32 = rows.view(np.int32)
    i32[:, 2 * MASK_WORD] = g.integers(0, 1 << 28, n)
    i32[:, 2 * MASK_WORD + 1] = g.integers(0, 1000, n)
    if not robot12:                                     # joints 8..11 of a Solo8 row are not joints: whatever they hold stays
        rows[:, W("q") + 8:W("q") + 12] = g.uniform(-50, 50, (n, 4))
    return rows


def crafted_rows(robot12):
    """rows that meet the table's corners -> (rows, names): the standing pose, -0.0 members, joints at the clamp, a base far above and
    far below the ground, upside down"""
    rows, names = [], []

    def add(name, **words):
        r = random_rows(robot12, 1, 1000 + len(rows))[0]
        r[W("pos"):W("pos") + 3] = (0.0, 0.0, 0.35)
        r[QUAT] = (0.0, 0.0, 0.0, 1.0)
        r[W("q"):W("q") + (12 if robot12 else 8)] = 0.0
        for k, v in words.items():
            member, idx = k.rsplit("_", 1)
            r[W(member) + int(idx)] = v
        rows.append(r)
        names.append(name)

    add("reset pose")
    add("negative zeros", q_0=-0.0, qd_1=-0.0, lin_vel_0=-0.0, lin_vel_2=-0.0, ang_vel_1=-0.0, quat_0=-0.0, pos_2=-0.0)
    add("joints at the upper clamp", q_0=0.95, q_3=1.0, q_7=0.99)
    add("joints at the lower clamp", q_1=-0.95, q_4=-1.0, q_6=-0.99)
    add("joint beyond the clamp", q_2=5.0, q_5=-5.0)
    add("far above the ground", pos_2=3.0)
    add("far below the ground", pos_2=-3.0)
    add("upside down", quat_0=1.0, quat_3=0.0)
    add("on its side", quat_0=math.sqrt(0.5), quat_3=math.sqrt(0.5))
    add("quaternion not normalised, w < 0", quat_0=0.2, quat_1=-0.4, quat_2=0.6, quat_3=-2.0)
    return np.stack(rows), names


def batch(robot12, n, seed=7):
    """the crafted rows, then random ones, n in all (n smaller than the crafted set: its first n) -> rows [n, 255]"""
    c, _ = crafted_rows(robot12)
    if n <= len(c):
        return c[:n].copy()
    return np.concatenate([c, random_rows(robot12, n - len(c), seed)])


def check(got_rows, got_count, want_rows, want_count, rows_in, mask=None, live=None, what=""):
    """got against want: every word outside quat and pos.z bit for bit, those two to TOL_TRIG (rows of ``live`` only; a row that is not
    live is not compared); every word outside the written set and every masked row bit for bit what went in"""
    n = rows_in.shape[0]
    sel = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    cmp = sel if live is None else sel & np.asarray(live, bool)
    assert np.array_equal(got_count, want_count), (what, "count", got_count[:8], want_count[:8])
    gb, wb, ib = bits(got_rows), bits(want_rows), bits(rows_in)
    assert np.array_equal(gb[~sel], ib[~sel]), (what, "a masked row was written")
    assert np.array_equal(gb[:, ~WRITTEN], ib[:, ~WRITTEN]), (what, "a word outside the written set was written", np.argwhere(gb[:, ~WRITTEN] != ib[:, ~WRITTEN])[:4])
    exact = gb[cmp][:, ~APPROX] == wb[cmp][:, ~APPROX]
    assert exact.all(), (what, "bitwise members", np.argwhere(~exact)[:6])
    err = np.abs(got_rows[cmp][:, APPROX] - want_rows[cmp][:, APPROX])
    assert err.size == 0 or float(err.max()) <= TOL_TRIG, (what, "quat / pos.z", float(err.max()))
    return float(err.max()) if err.size else 0.0


# ---------------------------------------------------------------- the host program (tests/host/reset_random_main.cpp)
def host_reset(exe, robot12, p, rows, count, mask=None, check_params=False):
    """one call of the host program -> (rows [n, 255], count [n] uint32) after it, or None if ``check_params`` and the parameters are
    refused"""
    n = rows.shape[0]
    hx64 = hex64
    text = ["%d %d %s %d %d" % (1 if robot12 else 0, n, hx64([p.joint_limit]), int(check_params), int(mask is not None)),
            "%d %d %d" % (p.seed, p.id0, p.place_on_ground), hx64(p.doubles())]
    if mask is not None:
        text.append(" ".join(str(int(b)) for b in np.asarray(mask, dtype=np.uint8)))
    text.append(" ".join(str(int(c)) for c in count))
    text += [hx64(rows[i]) for i in range(n)]
    lines = run_host(exe, input="\n".join(text) + "\n").strip().split("\n")
    if lines[0] == "refused":
        return None
    assert len(lines) == 1 + n, len(lines)
    cnt = np.array([int(x) for x in lines[0].split()], dtype=np.uint32)
    out = np.array([[int(x, 16) for x in line.split()] for line in lines[1:]], dtype=np.uint64).view(np.float64)
    return out, cnt
