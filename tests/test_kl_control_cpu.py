"""PPO KL control as far as a machine without a GPU sees it: the rule as a pure function, the eager PPO.update that applies it on
recipe R (tests/kl_util.py), the refusals of the two _kl entry points, the training flags, and the built kernels' resource records."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from solorl_amd import _native, build
from solorl_amd.ppo.kl_control import kl_rule
from solorl_amd.ppo.ppo import PPO

from . import kl_util as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


# (kl, lr, stopped before, desired_kl, target_kl) -> (lr, stopped); lr_factor 1.5, bounds [1e-5, 1e-2]
RULE_TABLE = [
    ((0.05, 1e-3, False, 0.01, None), (F(1e-3) / F(1.5), False)),                 # shrink
    ((0.001, 1e-3, False, 0.01, None), (F(1e-3) * F(1.5), False)),                # grow
    ((0.01, 1e-3, False, 0.01, None), (F(1e-3), False)),                          # hold: between desired / 2 and 2 desired
    ((0.02, 1e-3, False, 0.01, None), (F(1e-3), False)),                          # ... the upper threshold itself holds (f32: 2 * 0.01f)
    ((0.05, 1.2e-5, False, 0.01, None), (F(1e-5), False)),                        # the lower clamp
    ((0.001, 9e-3, False, 0.01, None), (F(1e-2), False)),                         # the upper clamp
    ((0.0, 1e-3, False, 0.01, None), (F(1e-3), False)),                           # kl = 0 does not grow
    ((-1e-4, 1e-3, False, 0.01, None), (F(1e-3), False)),                         # nor does a negative one
    ((float("nan"), 1e-3, False, 0.01, 0.01), (F(1e-3), False)),                  # not finite: nothing changes, nothing stops
    ((float("inf"), 1e-3, False, 0.01, 0.01), (F(1e-3), False)),
    ((-float("inf"), 1e-3, False, 0.01, 0.01), (F(1e-3), False)),
    ((0.05, 1e-3, False, None, None), (F(1e-3), False)),                          # control off
    ((0.05, 1e-3, False, 0.0, 0.0), (F(1e-3), False)),
    ((0.016, 1e-3, False, None, 0.01), (F(1e-3), True)),                          # stop above 1.5 target_kl
    ((0.014, 1e-3, False, None, 0.01), (F(1e-3), False)),
    ((0.001, 1e-3, True, 0.01, 0.01), (F(1e-3), True)),                           # stopped stays stopped, and the rate is left alone
    ((0.05, 1e-3, False, 0.01, 0.01), (F(1e-3), True)),                           # the stop is decided first: no shrink on that step
    ((0.012, 1e-3, False, 0.005, 0.01), (F(1e-3) / F(1.5), False)),               # both on, below the stop: shrink
]


def test_rule_table():
    for (kl, lr, stopped, d, t), (lr_want, stop_want) in RULE_TABLE:
        lr_got, stop_got = kl_rule(kl, lr, stopped, d, t)
        assert lr_got.dtype == np.float32 and R.f32_bits(lr_got) == R.f32_bits(lr_want) and stop_got is stop_want, (kl, lr, stopped, d, t, lr_got, stop_got)
    # the quotient, not the product with a reciprocal: from 1.9753088e-4 (four cuts below 1e-3) they differ in the last bit
    lr = F(1e-3) / F(1.5) / F(1.5) / F(1.5) / F(1.5)
    assert lr / F(1.5) != lr * (F(1.0) / F(1.5)) and kl_rule(0.05, lr, desired_kl=0.01)[0] == lr / F(1.5)
    assert kl_rule(0.05, 1e-3, desired_kl=0.01, lr_factor=2.0)[0] == F(1e-3) / F(2.0)
    assert kl_rule(0.05, 1e-3, desired_kl=0.01, lr_min=8e-4)[0] == F(8e-4)


def _run(**kw):
    """eager PPO on recipe R, with the parameters in front of every optimizer step -> (agent, policy, storage, returned, snapshots)"""
    pol = R.recipe_policy()
    st = R.recipe_storage(pol)
    args = list(R.PPO_ARGS)
    if "epochs" in kw:
        args[1] = kw.pop("epochs")
    agent = PPO(pol, *args, **R.PPO_KW, **kw)
    snaps = []
    agent.optimizer.register_step_pre_hook(lambda *_a: snaps.append(R.snapshot(pol)))
    torch.manual_seed(11)
    ret = agent.update(st)
    return agent, pol, st, ret, snaps


def _replay(log, desired_kl=None, target_kl=None, lr0=R.LR, kls=None):
    """the rule on a log's KLs (or on `kls` in their place) -> [(lr bits, applied)]"""
    lr, stopped, out = F(lr0), False, []
    for i, row in enumerate(log):
        lr, stopped = kl_rule(row[0] if kls is None else kls[i], lr, stopped, desired_kl, target_kl)
        out.append((int(R.f32_bits(lr)), 0.0 if stopped else 1.0))
    return out


def test_eager_ppo_adapts_the_learning_rate_on_recipe_R():
    agent, pol, st, _ret, snaps = _run(desired_kl=0.01)
    log = agent.last_step_log
    assert log.shape == (8, 4) and len(snaps) == 8
    kls = [R.kl64(pol, s, st) for s in snaps]
    print("KL per step, f64:", kls, "\nlogged:", log.tolist())
    R.assert_margins(kls, desired_kl=0.01)
    for k32, k in zip(log[:, 0].tolist(), kls):
        assert abs(k32 - k) <= R.bound(k), (k32, k)
    got = [(int(R.f32_bits(r[2])), float(r[3])) for r in log.numpy()]
    assert got == _replay(log.numpy(), 0.01) == _replay(log.numpy(), 0.01, kls=kls)      # the f64 KLs take the same decisions
    # what the decisions were: one growth, then seven cuts
    lrs = log[:, 2].numpy()
    assert lrs[0] > F(R.LR) and all(lrs[i + 1] < lrs[i] for i in range(7))
    d = agent.last_diagnostics
    assert d["steps"] == d["steps_applied"] == 8 and d["stopped"] is False
    assert R.f32_bits(d["lr"]) == R.f32_bits(lrs[-1]) and abs(d["lr"] - 8.7792e-05) < 1e-8
    assert math.isclose(d["approx_kl"], float(np.mean(log[:, 0].numpy(), dtype=np.float64)), rel_tol=1e-6)
    assert 0.0 <= d["clip_fraction"] <= 1.0 and d["clip_fraction"] == pytest.approx(float(log[:, 1].double().mean()), rel=1e-6)
    assert agent.optimizer.param_groups[0]["lr"] == float(lrs[-1])
    # a second update starts from a cleared state, at the rate the first one left
    agent.update(st)
    assert agent.last_diagnostics["steps"] == 8 and agent.last_step_log.shape == (8, 4)
    assert [r[0] for r in _replay(agent.last_step_log.numpy(), 0.01, lr0=lrs[-1])] == [int(R.f32_bits(x)) for x in agent.last_step_log[:, 2].numpy()]


def test_eager_ppo_stops_on_target_kl_on_recipe_R():
    agent, pol, st, _ret, snaps = _run(target_kl=0.01)
    d, log = agent.last_diagnostics, agent.last_step_log
    assert d["steps"] == 2 and d["steps_applied"] == 1 and d["stopped"] is True and log.shape == (2, 4)
    assert log[:, 3].tolist() == [1.0, 0.0] and len(snaps) == 1
    kls = [R.kl64(pol, snaps[0], st), R.kl64(pol, R.snapshot(pol), st)]          # (nothing moved after the stop: the parameters of step 1 are the final ones)
    R.assert_margins(kls, target_kl=0.01)
    for k32, k in zip(log[:, 0].tolist(), kls):
        assert abs(k32 - k) <= R.bound(k), (k32, k)
    assert kls[1] > 2.0 * 0.015                                                  # far beyond the stop threshold
    assert d["lr"] == float(F(R.LR))
    # the update that stopped after one step = one epoch without control, bit for bit
    _a1, pol1, _st, _r, _s = _run(epochs=1)
    for p, q in zip(pol.parameters(), pol1.parameters()):
        assert torch.equal(p, q)


def _todays_update(pol, st):
    """PPO.update as it was before KL control existed (agents/ppo/ppo.py:34-89), written out"""
    from solorl_amd.ppo import dist as D
    clip, epochs, mb, vc, ec = R.PPO_ARGS
    opt = torch.optim.Adam(pol.parameters(), lr=R.LR, weight_decay=0.0)
    bucket = D.FlatGradBucket(pol.parameters())
    adv = st.returns[:-1] - st.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    stats, n = torch.zeros(3), 0
    for _ in range(epochs):
        for obs_b, act_b, vpred_b, ret_b, _m, old_lp_b, adv_b in st.batch_generator(adv, mb):
            values, logp, entropy = pol.evaluate_actions(obs_b, act_b)
            ratio = torch.exp(logp - old_lp_b)
            action_loss = -torch.min(ratio * adv_b, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_b).mean()
            v_clipped = vpred_b + (values - vpred_b).clamp(-clip, clip)
            value_loss = 0.5 * torch.max((values - ret_b).pow(2), (v_clipped - ret_b).pow(2)).mean()
            bucket.zero()
            (value_loss * vc + action_loss - entropy * ec).backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), R.PPO_KW["max_grad_norm"])
            opt.step()
            stats += torch.stack([value_loss.detach(), action_loss.detach(), entropy.detach()])
            n += 1
    return tuple((stats / n).tolist())


def test_without_the_new_arguments_nothing_changes():
    agent, pol, st, ret, _snaps = _run()
    assert agent.last_diagnostics is None and agent.last_step_log is None and agent.kl.on is False
    pol0 = R.recipe_policy()
    torch.manual_seed(11)
    ret0 = _todays_update(pol0, R.recipe_storage(pol0))
    assert tuple(ret) == ret0
    for p, q in zip(pol.parameters(), pol0.parameters()):
        assert torch.equal(p, q)
    # measuring alone moves nothing either
    agent_d, pol_d, _st, ret_d, _s = _run(diagnostics=True)
    assert tuple(ret_d) == ret0 and agent_d.last_diagnostics["steps"] == 8 and agent_d.optimizer.param_groups[0]["lr"] == R.LR
    for p, q in zip(pol_d.parameters(), pol0.parameters()):
        assert torch.equal(p, q)
    with pytest.raises(ValueError):
        PPO(R.recipe_policy(), *R.PPO_ARGS, **R.PPO_KW, desired_kl=0.01, lr_factor=1.0)
    with pytest.raises(ValueError):
        PPO(R.recipe_policy(), *R.PPO_ARGS, **R.PPO_KW, desired_kl=0.01, lr_bounds=(1e-2, 1e-5))


# ---------------------------------------------------------------------------------------------------------------- the entry points
def _tables(obs_dim, act_dim, hidden=64, critic_obs_dim=0):
    P = _native.PolicyParams()
    P.obs_dim, P.act_dim, P.hidden, P.critic_obs_dim = obs_dim, act_dim, hidden, critic_obs_dim
    for k, _t in P._fields_[4:]:
        setattr(P, k, 4096)                           # non-null, 16-byte aligned (never dereferenced on the host)
    B, W, G, S, K = _native.PpoBatch(), _native.PpoStage1(), _native.PpoGrads(), _native.AdamState(), _native.KlControl()
    for st in (B, W, G, S, K):
        for k, t in st._fields_:
            if t is C.c_void_p:
                setattr(st, k, 4096)
    B.m = K.m = S.offset_increment = 64
    K.desired_kl, K.lr_factor, K.lr_min, K.lr_max, K.target_kl, K.log_capacity = 0.01, 1.5, 1e-5, 1e-2, 0.0, 8
    return P, B, W, G, S, K


D4096 = C.c_void_p(4096)
S1, CA = "solorl_ppo_grad_stage1_kl", "solorl_ppo_clip_adam_kl"


def _stage1(lib, P, B, W, critic=False, diag=D4096, generic=0):
    c = D4096 if critic else None
    return lib.solorl_ppo_grad_stage1_kl(C.byref(P) if P is not None else None, C.byref(B) if B is not None else None, c,
                                         C.byref(W) if W is not None else None, c, diag, generic, 0, None)


def _adam(lib, P, G, S, K, generic=0):
    ref = lambda x: C.byref(x) if x is not None else None
    return lib.solorl_ppo_clip_adam_kl(ref(P), ref(G), ref(S), ref(K), generic, 0, None)


def _refused(lib, rc, name, what):
    msg = lib.solorl_last_error()
    assert rc == -1 and msg.startswith(name.encode() + b": ") and what in msg, (rc, msg)


@pytest.mark.parametrize("generic,shape", [(0, (76, 0, 12)), (0, (76, 96, 12)), (1, (79, 0, 12)), (1, (79, 96, 12))])
def test_kl_entry_points_refuse_by_name_before_the_device(lib, generic, shape):
    o, oc, a = shape
    crit = oc != 0
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    # what is new: a null diag / state / lr, another lr than Adam's, another m than the batch's, the factor, the bounds
    _refused(lib, _stage1(lib, P, B, W, crit, diag=None, generic=generic), S1, b"null diag")
    for field in ("diag", "state", "lr"):
        P, B, W, G, S, K = _tables(o, a, 64, oc)
        setattr(K, field, None)
        _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"null diag, state or lr")
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    _refused(lib, _adam(lib, P, G, S, None, generic), CA, b"null argument")
    K.lr = 8192
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"k->lr must be a->lr")
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    K.m = 128
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"k->m is not the batch's m")
    K.m = 48
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"multiple of 32")
    for factor in (1.0, 0.5, float("nan")):
        P, B, W, G, S, K = _tables(o, a, 64, oc)
        K.lr_factor = factor
        _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"lr_factor must be > 1")
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    K.lr_min, K.lr_max = 1e-2, 1e-5
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"lr_min must not exceed lr_max")
    # what the plain entry points refuse
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    _refused(lib, _stage1(lib, None, B, W, crit, generic=generic), S1, b"null policy parameters")
    _refused(lib, _adam(lib, None, G, S, K, generic), CA, b"null policy parameters")
    _refused(lib, _stage1(lib, P, None, W, crit, generic=generic), S1, b"null argument or m < 1")
    _refused(lib, _adam(lib, P, None, S, K, generic), CA, b"null argument")
    _refused(lib, _stage1(lib, P, B, W, not crit, generic=generic), S1, b"critic_obs_dim is 0" if not crit else b"critic's arrays are NULL")
    B.m = 48
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"multiple of 32")
    B.m = 1 << 25
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"indexed with 32 bits")
    B.m = 64
    W.partials = None
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"null array")
    P, B, W, G, S, K = _tables(o, a, 64, oc)
    P.mean_w = None
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"null policy parameter pointer")
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"null policy parameter pointer")
    P, B, W, G, S, K = _tables(o, a, 32, oc)
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"64")
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"64")
    # a shape outside the family the switch picks
    P, B, W, G, S, K = _tables(129 if generic else 79, a, 64, oc)
    _refused(lib, _stage1(lib, P, B, W, crit, generic=generic), S1, b"SOLORL_POLICY_MAX_WIDTH = 128" if generic else b"policy kernels are built for")
    _refused(lib, _adam(lib, P, G, S, K, generic), CA, b"SOLORL_POLICY_MAX_WIDTH = 128" if generic else b"policy kernels are built for")
    # ... and with every argument in order the device is looked up, last (without one: no fall-back; with one the dummies must not be launched on)
    if not torch.cuda.is_available():
        P, B, W, G, S, K = _tables(o, a, 64, oc)
        for call, name in ((lambda: _stage1(lib, P, B, W, crit, generic=generic), S1), (lambda: _adam(lib, P, G, S, K, generic), CA)):
            rc, msg = call(), lib.solorl_last_error()
            assert rc == -2 and msg.startswith(name.encode() + b": ") and b"no CPU fallback" in msg, (rc, msg)


def test_the_struct_is_the_headers_and_the_abi_version_stays(lib):
    hdr = open(build.INC[0]).read()
    m = re.search(r"typedef struct solorl_kl_control \{(.*?)\} solorl_kl_control;", hdr, re.S)
    names = re.findall(r"\b(diag|m|desired_kl|lr_factor|lr_min|lr_max|target_kl|lr|state|log|log_capacity)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [k for k, _ in _native.KlControl._fields_]
    assert C.sizeof(_native.KlControl) == 64 and _native.KlControl.lr.offset == 32 and _native.KlControl.log_capacity.offset == 56
    assert "#define SOLORL_ABI_VERSION 5\n" in hdr and lib.solorl_abi_version() == 5


# ---------------------------------------------------------------------------------------------------------------- the training flags
def _args(argv):
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_ppo
    a = train_ppo.get_ppo_args(argv)
    a.cuda = False
    return a


def test_train_refuses_flag_combinations(monkeypatch):
    from solorl_amd.ppo import train as T
    with pytest.raises(ValueError, match="--desired-kl with --use-linear-lr-decay"):
        T.train(_args(["--desired-kl", "0.01", "--use-linear-lr-decay"]), {})
    monkeypatch.setattr(T.D, "init_from_env", lambda *_a, **_k: (0, 2))
    for flags in (["--desired-kl", "0.01"], ["--target-kl", "0.02"], ["--ppo-diagnostics"]):
        with pytest.raises(NotImplementedError, match="single process"):
            T.train(_args(flags), {})


def test_train_script_flags_reach_train(monkeypatch):
    from solorl_amd.ppo import train as T
    seen = {}
    monkeypatch.setattr(T, "train", lambda args, config, *rest: seen.update(args=args) or "called")
    monkeypatch.syspath_prepend(ROOT)
    import train_ppo
    cfg = os.path.join(ROOT, "configs", "basic12.yaml")
    assert train_ppo.main(["--config-file", cfg, "--desired-kl", "0.01", "--target-kl", "0.03", "--ppo-diagnostics"]) == "called"
    a = seen["args"]
    assert (a.desired_kl, a.target_kl, a.ppo_diagnostics) == (0.01, 0.03, True)
    d = train_ppo.get_ppo_args([])
    assert (d.desired_kl, d.target_kl, d.ppo_diagnostics) == (None, None, False)


# ---------------------------------------------------------------------------------------------------------------- the built code
DIMS = [(76, 76, 12), (84, 84, 12), (38, 38, 12), (42, 42, 12), (60, 60, 8), (68, 68, 8), (30, 30, 8), (34, 34, 8), (41, 41, 12), (45, 45, 12),
        (33, 33, 8), (37, 37, 8), (38, 58, 12), (41, 58, 12), (76, 96, 12), (30, 50, 8), (33, 50, 8), (60, 80, 8)]


def test_new_kernels_use_no_scratch_and_the_existing_ones_are_all_there(lib):
    from solorl_amd import devcode
    res = devcode.kernel_resources(build.LIB)
    t3 = lambda d: "ILi%dELi%dELi%dEE" % d
    new, old = [], []
    for d in DIMS:
        new += ["ppo_grad_stage1_kl_kernel" + t3(d), "ppo_clip_adam_kl_kernel" + t3(d)]
        old += ["ppo_grad_stage1_mfma_kernel" + t3(d), "ppo_clip_adam_kernel" + t3(d), "policy_act_mfma_kernel" + t3(d)]
    for a in (8, 12):
        new += ["ppo_grad_stage1_w_kl_kernelILi%dEE" % a, "ppo_clip_adam_w_kl_kernelILi%dEE" % a]
        old += ["ppo_grad_stage1_w_kernelILi%dEE" % a, "ppo_clip_adam_w_kernelILi%dEE" % a, "policy_act_w_kernelILi%dEE" % a]
    old += ["ppo_grad_stage2_mfma_kernelILb0EE", "ppo_grad_stage2_mfma_kernelILb1EE", "ppo_grad_stage3_kernel"]
    find = lambda part: [k for k in res if part in k]
    for part in old:
        assert len(find(part)) == 1, part
    for part in new:
        ks = find(part)
        assert len(ks) == 1, part
        assert res[ks[0]]["private_segment_fixed_size"] == 0, (part, res[ks[0]])
    # the plain twins keep what they had: no scratch, and stage 1's two workgroups per CU (at most 128 registers a lane, AGPRs included)
    for d in DIMS:
        for part in ("ppo_grad_stage1_mfma_kernel" + t3(d), "ppo_grad_stage1_kl_kernel" + t3(d)):
            r = res[find(part)[0]]
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_count"] + r.get("agpr_count", 0) <= 256, (part, r)
