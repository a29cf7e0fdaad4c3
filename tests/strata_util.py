"""Shared by tests/test_strata_cpu.py and tests/test_strata_gpu.py: parity with the fp64 oracle PER STRATUM -- per number of solved
contacts, of joint-limit rows, per base orientation, per primitive in contact -- on a seeded bank of states in which fallen robots are as
common as standing ones.

  * bank(robot): at most BANK_MAX float32-representable states with one action row each, made with the oracle alone on the CPU from
    termination-disabled rollouts (inverted, on-side, nose-down, dropped and lying starts mixed in, joints pushed beyond their limits in a
    share of them), selected so that every stratum is populated.  Once per process, never modified.
  * reference(robot, level): the capped oracle's (set_caps(8, 4)) result of ONE control step ("step") or one physics sub-step ("substep")
    from every bank state, the strata read from ITS counts, and the yardstick: s_12 / s_24, the largest change of the compared quantity
    over three oracle twins whose start states are perturbed by 1e-12 / 2^-24 relative.  Nothing of the engine enters.
  * check_f64 / check_f32: the two criteria, per stratum, with the failure message that names the stratum and its worst samples.

The compared quantity is max | . | over pos, quat, lin_vel, ang_vel, q, qd and the lambda_prev of the primitives the reference has in
contact; beside it the contact mask (strip bits included) and, at step level, the reward."""
import ctypes as C
import json
import os

import numpy as np

from solorl_amd.config import EnvState, config_from_dict, default_config, load_yaml, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
from tests.util import GOLDEN, PARITY_MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = {"solo12": ROBOT_SOLO12, "solo8": ROBOT_SOLO8}
ROW_BYTES = C.sizeof(EnvState)
ROW_WORDS = ROW_BYTES // 8
N_CONT = EnvState.timestep.offset // 8        # the continuous members (all double) come first, the four int32 after them
assert EnvState.timestep.offset % 8 == 0 and ROW_BYTES - EnvState.timestep.offset == 16
BANK_MAX = 2048
SEED = 20250314
EPS_12, EPS_24, EPS_F64 = 1e-12, 2.0 ** -24, 1e-15
RHO_FLOOR = 1e-7                              # rho = e / max(s_24, RHO_FLOOR): fp32 rounding of O(1) members
MIN_STRATUM, MIN_PRIM, MIN_STRIP = 100, 50, 200
MEASURED = os.path.join(GOLDEN, "strata_measured.json")

# the pool: POOL_ENVS oracle envs rolled out for POOL_STEPS control steps, placed anew every POOL_REPLACE steps
POOL_ENVS, POOL_STEPS, POOL_REPLACE = 128, 96, 32
LYING_Z = (0.020, 0.025)                      # tests/test_helper_base_gpu.py: base level on its belly, every leg folded to its limits


def threads():
    try:
        return min(16, len(os.sched_getaffinity(0)))
    except AttributeError:
        return 4


def bank_cfg(robot):
    """Solo12: default walk.  Solo8: configs/basic.yaml (treadmill strip on).  Termination off, episodes that never time out."""
    c = default_config(ROBOT_SOLO12, TASK_WALK) if robot == ROBOT_SOLO12 else config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic.yaml")))
    assert c.robot == robot and c.task == TASK_WALK and c.use_treadmill == (robot == ROBOT_SOLO8)
    c.disable_termination = 1
    c.episode_length = 1000000
    c.num_history_stack = 1
    return c


def nprims(robot):
    return len(json.load(open(os.path.join(ROOT, "solorl_amd", "models", "solo12.json" if robot == ROBOT_SOLO12 else "solo8.json")))["prims"])


# ---------------------------------------------------------------- rows: states as one float64 [N, ROW_WORDS] array
def col(rows, name):
    """view of member `name` of solorl_env_state in rows [N, ROW_WORDS] (float64; the int32 members as int32 [N])"""
    f = getattr(EnvState, name)
    if name in ("timestep", "need_reset", "contact_mask", "rng_counter"):
        return rows.view(np.int32)[:, f.offset // 4]
    return rows[:, f.offset // 8: (f.offset + f.size) // 8]


def get_rows(orc):
    rows = np.zeros((orc.N, ROW_WORDS))
    for i in range(orc.N):
        orc.L.oracle_get_state(orc.h, i, C.c_void_p(rows.ctypes.data + i * ROW_BYTES))
    return rows


def set_rows(orc, rows):
    assert rows.shape == (orc.N, ROW_WORDS) and rows.dtype == np.float64 and rows.flags.c_contiguous
    for i in range(orc.N):
        orc.L.oracle_set_state(orc.h, i, C.c_void_p(rows.ctypes.data + i * ROW_BYTES))


def up_z(rows):
    """base z axis . world z"""
    q = col(rows, "quat")
    return 1.0 - 2.0 * (q[:, 0] ** 2 + q[:, 1] ** 2) / (q ** 2).sum(1)


def perturbed(rows, eps, seed):
    """every continuous member times 1 + eps u, u ~ U(-1, 1)"""
    out = rows.copy()
    out[:, :N_CONT] *= 1.0 + eps * np.random.default_rng(seed).uniform(-1, 1, (rows.shape[0], N_CONT))
    return out


def oracle_step(cfg, rows, actions):
    """one step of the capped oracle from `rows` -> (rows after, rewards, last_counts [N, 4])"""
    from oracle.oracle_py import Oracle
    orc = Oracle(cfg, rows.shape[0], seed=1, threads=threads())
    orc.set_caps(8, 4)
    set_rows(orc, rows)
    _, rew, done, _ = orc.step(actions.astype(np.float64))
    assert not done.any()
    return get_rows(orc), rew, np.array([orc.last_counts(i) for i in range(orc.N)])


# ---------------------------------------------------------------- the bank
def _quat_x(a):
    return [np.sin(a / 2), 0.0, 0.0, np.cos(a / 2)]


def _quat_y(a):
    return [0.0, np.sin(a / 2), 0.0, np.cos(a / 2)]


def _place(rows, cfg, rng):
    """the start poses of the issue, by env index modulo 16: 0..3 stay as they are (_pool puts 0 and 1 back into the reset crouch, 2 and 3 go on from whatever
    they reached); the others are dropped at rest from z = 0.35 inverted (about x, +-0.2 rad), on either side, nose or tail down, from 1 m as
    they are, or laid on the belly with folded legs"""
    n, ql = cfg.n_joints, float(cfg.joint_limit)
    fold = [0.0, ql, -ql] * 4 if n == 12 else [ql, -ql] * 4
    for i in range(rows.shape[0]):
        k = i % 16
        if k < 4:
            continue
        r = rows[i:i + 1]
        col(r, "lin_vel")[:] = 0; col(r, "ang_vel")[:] = 0; col(r, "qd")[:] = 0
        if k < 13:
            col(r, "pos")[0, 2] = 0.35
            col(r, "q")[0, :n] = rng.uniform(-1.5, 1.5, n)
            if k < 7:
                col(r, "quat")[0] = _quat_x(np.pi + rng.uniform(-0.2, 0.2))
            elif k < 10:
                col(r, "quat")[0] = _quat_x((1 if i // 16 % 2 else -1) * np.pi / 2 + rng.uniform(-0.1, 0.1))
            else:
                col(r, "quat")[0] = _quat_y((1 if i // 16 % 2 else -1) * np.pi / 2 + rng.uniform(-0.1, 0.1))
        elif k == 13:
            col(r, "pos")[0, 2] = 1.0
        else:
            # (not exactly level and not exactly at the limits: four belly corners at the same depth to the last bit are a tie of the
            # cap's "deepest 8", and q = limit a tie of the limit test, which any perturbation of the state decides anew)
            col(r, "pos")[0, 2] = LYING_Z[i // 16 % 2] + rng.uniform(0.0, 0.004)
            qx, qy = _quat_x(rng.uniform(-0.03, 0.03)), _quat_y(rng.uniform(-0.03, 0.03))
            col(r, "quat")[0] = [qx[0] * qy[3], qx[3] * qy[1], -qx[0] * qy[1], qx[3] * qy[3]]
            col(r, "q")[0, :n] = np.array(fold) + np.sign(fold) * rng.uniform(0.0, 0.05, n)
            col(r, "lambda_prev")[:] = 0


def _pool(cfg):
    """-> (states [P, ROW_WORDS], actions [P, n] float32): every state of the rollouts with the action that followed it"""
    from oracle.oracle_py import Oracle
    rng = np.random.default_rng(SEED + cfg.robot)
    n = cfg.n_joints
    orc = Oracle(cfg, POOL_ENVS, seed=SEED, threads=threads())
    orc.set_caps(8, 4)
    orc.reset()
    back = np.arange(POOL_ENVS) % 16 < 2
    S, A = [], []
    for t in range(POOL_STEPS):
        rows = get_rows(orc)
        if t == 0:
            start = rows.copy()
        if t % POOL_REPLACE == 0:
            rows[back] = start[back]                # back to the reset crouch
            _place(rows, cfg, rng)
            set_rows(orc, rows)
        a = rng.uniform(-1, 1, (POOL_ENVS, n)).astype(np.float32)
        orc.step(a.astype(np.float64))
        S.append(rows); A.append(a)
    return np.concatenate(S), np.concatenate(A)


def _inject_limits(rows, cfg, rng, k):
    """k joints of every row beyond their limits with some speed (tests/test_parity_gpu2.py::test_joint_limit_rows_vs_oracle)"""
    n, ql = cfg.n_joints, float(cfg.joint_limit)
    for i in range(rows.shape[0]):
        for j in rng.choice(n, size=k, replace=False):
            col(rows, "q")[i, j] = rng.choice([-1, 1]) * (ql + rng.uniform(0.0, 0.3))
            col(rows, "qd")[i, j] = rng.uniform(-10, 10)


def strata_names(robot):
    return (["contacts %d" % k for k in range(9)] + ["cap binds"] + ["limit rows %d" % k for k in range(5)] + ["candidates > rows"]
            + ["upright", "on side", "inverted", "free flight"] + ["primitive %d" % p for p in range(nprims(robot))]
            + (["strip"] if robot == ROBOT_SOLO8 else []))


def _membership(robot, rows, mask_after, counts):
    """bool [N, S] in the order of strata_names: from the REFERENCE's counts and contact mask of the step and the start orientation"""
    found, solved, cand, lrows = counts.T
    uz = up_z(rows)
    m = [solved == k for k in range(9)] + [found > solved] + [lrows == k for k in range(5)] + [cand > lrows]
    m += [uz > 0.5, np.abs(uz) < 0.5, uz < -0.5, (found == 0) & (lrows == 0)]
    m += [(mask_after >> p) & 1 == 1 for p in range(nprims(robot))]
    if robot == ROBOT_SOLO8:
        m.append((mask_after >> 24) != 0)
    return np.stack(m, 1)


def _quota(name):
    return 1.3 * (MIN_PRIM if name.startswith("primitive") else MIN_STRIP if name == "strip" else MIN_STRATUM)


class Bank:
    pass


_BANKS, _REFS = {}, {}


def bank(robot):
    """The bank of `robot`: .cfg, .n, .rows [N, ROW_WORDS] float64 (every continuous member float32-representable), .actions [N, n]
    float32.  Built once per process; nobody writes to it."""
    if robot not in _BANKS:
        cfg = bank_cfg(robot)
        rng = np.random.default_rng(SEED + 100 + robot)
        S, A = _pool(cfg)
        names = strata_names(robot)
        # joints beyond their limits in copies of a share of the pool: 1..6 joints each
        for k in (1, 2, 3, 4, 5, 6):
            idx = rng.choice(S.shape[0], size=300, replace=False)
            r = S[idx].copy()
            _inject_limits(r, cfg, rng, k)
            S = np.concatenate([S, r]); A = np.concatenate([A, A[idx]])
        S[:, :N_CONT] = S[:, :N_CONT].astype(np.float32).astype(np.float64)       # every precision and the oracle start from the same numbers
        col(S, "tau")[:] = 0
        # the strata of every pool state, from the capped oracle's step of it: what reference() will find for the chosen ones
        after, _, counts = oracle_step(cfg, S, A)
        X = _membership(robot, S, col(after, "contact_mask"), counts)
        # stratum-balanced selection: the rarest stratum first, each filled to its quota from what is not yet chosen
        chosen = np.zeros(S.shape[0], bool)
        for s in np.argsort(X.sum(0)):
            short = int(_quota(names[s]) - (X[:, s] & chosen).sum())
            avail = np.flatnonzero(X[:, s] & ~chosen)
            if short > 0 and avail.size:
                chosen[rng.choice(avail, size=min(short, avail.size), replace=False)] = True
        assert chosen.sum() <= BANK_MAX, chosen.sum()
        rest = np.flatnonzero(~chosen)
        chosen[rng.choice(rest, size=min(BANK_MAX - int(chosen.sum()), rest.size), replace=False)] = True
        b = Bank()
        b.robot, b.cfg, b.n = robot, cfg, cfg.n_joints
        b.rows = np.ascontiguousarray(S[chosen])
        b.actions = np.ascontiguousarray(A[chosen])
        b.N = b.rows.shape[0]
        b.rows.setflags(write=False); b.actions.setflags(write=False)
        _BANKS[robot] = b
    return _BANKS[robot]


# ---------------------------------------------------------------- the reference result, its strata and the yardstick
def compared(rows, n, ref_mask):
    """[N, 13 + 2 n + 24]: pos, quat, lin_vel, ang_vel, q, qd, and lambda_prev of the primitives in contact in the reference"""
    lam = np.where((ref_mask[:, None] >> np.arange(24)) & 1, col(rows, "lambda_prev"), 0.0)
    return np.concatenate([col(rows, "pos"), col(rows, "quat"), col(rows, "lin_vel"), col(rows, "ang_vel"), col(rows, "q")[:, :n],
                           col(rows, "qd")[:, :n], lam], 1)


class Ref:
    def errors(self, rows, rew=None):
        """-> (e, e on q alone, reward error or None, contact masks) of a result `rows` against the reference"""
        d = np.abs(compared(rows, self.n, self.mask) - self.vec)
        return d.max(1), d[:, 13:13 + self.n].max(1), None if rew is None else np.abs(np.asarray(rew, np.float64) - self.rew), col(rows, "contact_mask").copy()


def level_cfg(cfg, level):
    c = cfg.copy()
    if level == "substep":                    # one control step of frame_skip 1 is one physics sub-step under the action's torque
        c.frame_skip = 1
    return c


def twin(robot, level, eps, seed):
    """the oracle's own result from the bank perturbed by eps -> (rows after, rewards)"""
    b = bank(robot)
    rows, rew, _ = oracle_step(level_cfg(b.cfg, level), perturbed(b.rows, eps, seed), b.actions)
    return rows, rew


def reference(robot, level="step"):
    """Once per process: the capped oracle's step (or sub-step) from the bank, .strata {name: bool [N]}, .counts [N, 4], .uz, and the
    yardstick .s12, .s24 (compared quantity), .s24_q (q alone), .s24_rew, .knife (a twin's contact mask differs from the reference's)."""
    if (robot, level) not in _REFS:
        b = bank(robot)
        cfg = level_cfg(b.cfg, level)
        r = Ref()
        r.robot, r.level, r.n, r.N = robot, level, b.n, b.N
        r.rows, r.rew, r.counts = oracle_step(cfg, b.rows, b.actions)
        r.mask = col(r.rows, "contact_mask").copy()
        r.vec = compared(r.rows, b.n, r.mask)
        r.uz = up_z(b.rows)
        X = _membership(robot, b.rows, r.mask, r.counts)
        r.strata = {name: X[:, k] for k, name in enumerate(strata_names(robot))}
        r.knife = np.zeros(b.N, bool)
        for name, eps in (("12", EPS_12), ("24", EPS_24)):
            s, sq, sr = np.zeros(b.N), np.zeros(b.N), np.zeros(b.N)
            for k in range(3):
                rows, rew = twin(robot, level, eps, SEED + 1000 * k + (1 if name == "12" else 2))
                e, eq, er, m = r.errors(rows, rew)
                s, sq, sr = np.maximum(s, e), np.maximum(sq, eq), np.maximum(sr, er)
                r.knife |= m != r.mask
            setattr(r, "s" + name, s); setattr(r, "s%s_q" % name, sq); setattr(r, "s%s_rew" % name, sr)
        r.calibration = r.strata["upright"] & (r.counts[:, 1] <= 4) & (r.counts[:, 3] <= 1)
        _REFS[(robot, level)] = r
    return _REFS[(robot, level)]


def rho(ref, e):
    return e / np.maximum(ref.s24, RHO_FLOOR)


def quantiles(x):
    x = np.asarray(x, np.float64)
    return {"n": int(x.size), "p50": float(np.percentile(x, 50)), "p90": float(np.percentile(x, 90)), "p99": float(np.percentile(x, 99))}


# ---------------------------------------------------------------- the criteria
def worst(ref, sel, e, s, masks, k=5):
    """the failure message's table: the k samples of `sel` with the largest e / s"""
    idx = np.flatnonzero(sel)
    idx = idx[np.argsort(-(e[idx] / np.maximum(s[idx], 1e-300)))][:k]
    return "\n".join("  bank %4d: contacts found %2d solved %d, limit candidates %d rows %d, base z . world z %+.3f, e %.3e, s %.3e, masks %08x / %08x (oracle)%s" % (
        i, ref.counts[i, 0], ref.counts[i, 1], ref.counts[i, 2], ref.counts[i, 3], ref.uz[i], e[i], s[i], int(masks[i]) & 0xFFFFFFFF, int(ref.mask[i]) & 0xFFFFFFFF,
        " knife-edge" if ref.knife[i] else "") for i in idx)


def allowed_exceptions(n):
    """criterion F64: 0.5 % of a stratum, at most 1 sample below 200 -- a discrete event (a residual exit one sweep apart, a contact at
    its threshold) that three twins can miss; the reference's own 1e-15 twin needed 1 in 15 360"""
    return 1 if n < 200 else int(0.005 * n)


def check_knife_edge(ref):
    for name, sel in ref.strata.items():
        assert (ref.knife & sel).sum() <= 0.01 * sel.sum(), "%s: stratum '%s' has %d knife-edge samples of %d" % (ref.level, name, (ref.knife & sel).sum(), sel.sum())


def check_f64(mode, ref, rows, median_q=True, exceptions=True):
    """Criterion F64 on a result `rows` [N, ROW_WORDS]: per sample e <= max(1e-12, s_12) (exceptions per stratum: allowed_exceptions, or
    none), contact masks and strip bits equal outside knife-edge samples, per-stratum median of e on q < 1e-13.  -> violations [N]"""
    e, eq, _, masks = ref.errors(rows)
    bound = np.maximum(1e-12, ref.s12)
    viol = e > bound
    flip = (masks != ref.mask) & ~ref.knife
    print("strata[%s] F64: e p50 %.2e p90 %.2e max %.2e; s_12 p50 %.2e; violations %d, mask differences outside knife-edge %d, knife-edge %d of %d" % (
        mode, np.median(e), np.percentile(e, 90), e.max(), np.median(ref.s12), viol.sum(), flip.sum(), ref.knife.sum(), ref.N))
    for name, sel in ref.strata.items():
        n = int(sel.sum())
        if n == 0:
            continue
        assert not (flip & sel).any(), "%s, stratum '%s': contact mask differs from the oracle's in %d samples that are not knife-edge\n%s" % (
            mode, name, (flip & sel).sum(), worst(ref, flip & sel, e, bound, masks))
        cap = allowed_exceptions(n) if exceptions else 0
        assert (viol & sel).sum() <= cap, "%s, stratum '%s': %d of %d samples above max(1e-12, s_12), %d allowed\n%s" % (
            mode, name, (viol & sel).sum(), n, cap, worst(ref, viol & sel, e, bound, masks))
        if median_q:
            assert np.median(eq[sel]) < 1e-13, "%s, stratum '%s': median |dq| %.3e >= 1e-13\n%s" % (mode, name, np.median(eq[sel]), worst(ref, sel, e, bound, masks))
    return viol


def check_reward(mode, ref, rows, rew):
    """the step's reward within max(1e-3, 30 s_24 of the reward) of the oracle's"""
    e, _, er, masks = ref.errors(rows, rew)
    bad = er > np.maximum(1e-3, 30 * ref.s24_rew)
    assert not bad.any(), "%s: reward off by more than max(1e-3, 30 s_24) in %d samples (e, s below: of the reward)\n%s" % (
        mode, bad.sum(), worst(ref, bad, er, np.maximum(ref.s24_rew, 1e-300), masks))


def stratum_quantiles(ref, r):
    return {name: quantiles(r[sel]) for name, sel in ref.strata.items() if sel.any()}


def check_f32(mode, ref, rows, rew, calibration):
    """Criterion F32 on a result: per stratum the p50 / p90 / p99 of rho = e / max(s_24, 1e-7) within PARITY_MARGIN x `calibration`
    ({"p50", "p90", "p99"}; p99 only from 300 samples on, as tests/util.py check_parity_stats); and, whatever the calibration says: no sample
    above 1e-3 rad on q unexplained (knife-edge, or s_24 on q above 1e-4), masks equal outside knife-edge samples in 98 % of every
    stratum, reward within max(1e-3, 30 s_24 of the reward)."""
    e, eq, er, masks = ref.errors(rows, rew)
    r = rho(ref, e)
    sden = np.maximum(ref.s24, RHO_FLOOR)
    flip = (masks != ref.mask) & ~ref.knife
    for name, sel in list(ref.strata.items()) + [("calibration", ref.calibration)]:
        n = int(sel.sum())
        if n == 0:
            continue
        assert (flip & sel).sum() <= 0.02 * n, "%s, stratum '%s': contact mask differs from the oracle's in %d of %d samples that are not knife-edge\n%s" % (
            mode, name, (flip & sel).sum(), n, worst(ref, flip & sel, e, sden, masks))
        q = quantiles(r[sel])
        for k in ("p50", "p90", "p99") if n >= 300 else ("p50", "p90"):
            assert q[k] <= PARITY_MARGIN * calibration[k], "%s, stratum '%s' (%d samples): %s of rho = %.3g exceeds %.1f x the calibration's %.3g\n%s" % (
                mode, name, n, k, q[k], PARITY_MARGIN, calibration[k], worst(ref, sel, e, sden, masks))
    # (after the strata, so that a fault confined to some of them is reported under their name)
    unexplained = (eq > 1e-3) & ~ref.knife & ~(ref.s24_q > 1e-4)
    assert not unexplained.any(), "%s: %d samples above 1e-3 rad on q that are neither knife-edge nor amplified by the oracle itself (s_24 on q <= 1e-4)\n%s" % (
        mode, unexplained.sum(), worst(ref, unexplained, eq, np.maximum(ref.s24_q, 1e-300), masks))
    check_reward(mode, ref, rows, rew)


# ---------------------------------------------------------------- measured figures
def stats_dir():
    """where a run leaves its figures: $SOLORL_STATS_DIR, or build/strata under the repository (git-ignored)"""
    return os.environ.get("SOLORL_STATS_DIR") or os.path.join(ROOT, "build", "strata")


def record(section, value):
    """strata_stats.json in stats_dir() collects what a run measured ("a/b/c" -> nested keys); tools/dev/collect_strata_stats.py copies
    it into tests/golden/strata_measured.json"""
    out = stats_dir()
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "strata_stats.json")
        cur = json.load(open(path)) if os.path.exists(path) else {}
        d = cur
        keys = section.split("/")
        for k in keys[:-1]:
            d = d.setdefault(k, {})
        d[keys[-1]] = value
        json.dump(cur, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def measured(section):
    """the entry "a/b/c" of tests/golden/strata_measured.json, or None"""
    d = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    for k in section.split("/"):
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d
