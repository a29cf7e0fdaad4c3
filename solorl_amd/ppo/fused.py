"""Fused PPO mini-batch loss (HIP kernel `solorl_ppo_loss`, include/solorl.h): the Gaussian log-prob, ratio,
clipped surrogate, clipped value loss and their gradients w.r.t. the policy heads in ONE launch instead of ~60
elementwise torch kernels (forward + autograd backward) per mini-batch.  Arithmetic of agents/ppo/ppo.py:52-74 and
agents/ppo/policy.py:51-58,171-173; torch's sub-gradient conventions for min/max/clamp.  GPU only."""
import ctypes as C
import math

import torch

from .. import _native

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class _FusedPPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, logstd, values, action, old_logp, adv, vpred, ret, clip, value_coef, entropy_coef, clipped_value):
        m, A = mean.shape
        dev = mean.device
        f = lambda x: x.detach().contiguous().float()
        mean_, logstd_, values_, action_ = f(mean), f(logstd), f(values).view(-1), f(action)
        old_, adv_, vpred_, ret_ = f(old_logp).view(-1), f(adv).view(-1), f(vpred).view(-1), f(ret).view(-1)
        nb = (m + 255) // 256
        g_mean = torch.empty_like(mean_)
        g_values = torch.empty_like(values_)
        part = torch.empty((nb, 3 + A), device=dev, dtype=torch.float32)
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            _native.check(_native.lib().solorl_ppo_loss(p(mean_), p(logstd_), p(values_), p(action_), p(old_), p(adv_), p(vpred_), p(ret_),
                                                        m, A, float(clip), float(value_coef), int(bool(clipped_value)), p(g_mean), p(g_values),
                                                        p(part), dev.index or 0, _native.stream(dev)))
        s = part.sum(0)
        value_loss, action_loss = s[0] / m, s[1] / m
        entropy = (0.5 + _HALF_LOG_2PI + logstd_).mean()
        loss = value_loss * value_coef + action_loss - entropy * entropy_coef
        ctx.save_for_backward(g_mean, g_values, s[3:] - entropy_coef / A)
        ctx.shapes = (mean.shape, logstd.shape, values.shape)
        ctx.mark_non_differentiable(value_loss, action_loss, entropy)
        return loss, value_loss, action_loss, entropy

    @staticmethod
    def backward(ctx, g, *_unused):
        g_mean, g_values, g_logstd = ctx.saved_tensors
        ms, ls, vs = ctx.shapes
        return (g_mean.view(ms) * g, g_logstd.view(ls) * g, g_values.view(vs) * g) + (None,) * 9


def fused_ppo_loss(mean, logstd, values, action, old_logp, adv, vpred, ret, clip, value_coef, entropy_coef, clipped_value=True):
    """-> (loss, value_loss, action_loss, entropy); loss = value_loss*value_coef + action_loss - entropy*entropy_coef."""
    return _FusedPPOLoss.apply(mean, logstd, values, action, old_logp, adv, vpred, ret, clip, value_coef, entropy_coef, clipped_value)


# ---------------------------------------------------------------------------------------------------------------------
# Hand-written policy kernels (csrc/solorl_ppo.hip): the whole forward of Policy.act in one launch, and one PPO mini-batch's
# gather + forward + losses + back-propagation in one launch (the weight gradients stay GEMMs).

# (obs, critic rows, act): csrc SOLO_DIMS_LIST.  The symmetric policy is critic rows = obs (zero or one history level, and zero history
# levels + the three command words of solorl_commands); then the shapes built with a critic width of its own
_SUPPORTED = {(76, 76, 12), (84, 84, 12), (38, 38, 12), (42, 42, 12), (60, 60, 8), (68, 68, 8), (30, 30, 8), (34, 34, 8),
              (41, 41, 12), (45, 45, 12), (33, 33, 8), (37, 37, 8),
              (38, 58, 12), (41, 58, 12), (76, 96, 12), (30, 50, 8), (33, 50, 8), (60, 80, 8)}


def policy_kernels_supported(actor_critic):
    """The kernels are built for the reference's default MLP (hidden 64, agents/ppo/policy.py:62-81) on zero or one history level."""
    b = actor_critic.base
    try:
        o, h, a = b.features[0].in_features, b.features[0].out_features, actor_critic.pi_dist.mean.out_features
    except AttributeError:
        return False
    p = next(actor_critic.parameters())
    oc = getattr(actor_critic, "critic_obs_dim", None)          # None: symmetric (a critic width that equals obs is not a built shape)
    if oc is not None and (oc == o or b.critic[0].in_features != oc):
        return False
    return h == 64 and (o, oc or o, a) in _SUPPORTED and p.is_cuda and p.dtype == torch.float32


def _policy_shape(actor_critic):
    """(obs, critic width or None for a symmetric policy, act, hidden) of the reference's MLP; None for another module"""
    b = actor_critic.base
    try:
        o, h, a = b.features[0].in_features, b.features[0].out_features, actor_critic.pi_dist.mean.out_features
        oc = getattr(actor_critic, "critic_obs_dim", None)
        if oc is not None and b.critic[0].in_features != oc:
            return None
    except AttributeError:
        return None
    return o, oc, a, h


def generic_shape_supported(o, oc, a, h=64):
    """The width-generic family (csrc/solorl_ppo.hip, the _w entry points): hidden 64, 8 or 12 actions, any observation width and any
    critic width (None: symmetric) up to SOLORL_POLICY_MAX_WIDTH; a critic width that equals obs is written None, as for the templates"""
    W = _native.POLICY_MAX_WIDTH
    return h == 64 and a in (8, 12) and 1 <= o <= W and (oc is None or (1 <= oc <= W and oc != o))


def policy_kernels_generic_supported(actor_critic):
    """policy_kernels_supported for the width-generic family"""
    shape = _policy_shape(actor_critic)
    p = next(actor_critic.parameters())
    return shape is not None and generic_shape_supported(*shape) and p.is_cuda and p.dtype == torch.float32


TEMPLATED, GENERIC = "templated", "generic"


def shape_kernel_family(o, oc, a, h=64, generic=0):
    """The kernel family for a policy shape (oc None: symmetric): TEMPLATED (one instance per shape, _SUPPORTED), GENERIC (the _w entry
    points) or None (the PyTorch path).  ``generic`` is the value of the switch SOLORL_POLICY_GENERIC (graphs.py reads it):
    0 the templated family or none, today's behaviour; 1 the generic family for the shapes the templated one does not build;
    2 the generic family for every shape it takes (A/B runs, the bitwise tests)."""
    templated = h == 64 and oc != o and (o, oc or o, a) in _SUPPORTED
    if generic and generic_shape_supported(o, oc, a, h) and (generic >= 2 or not templated):
        return GENERIC
    return TEMPLATED if templated else None


def policy_kernel_family(actor_critic, generic=0):
    """shape_kernel_family of a policy module whose parameters the kernels can read (CUDA, float32); None otherwise"""
    shape = _policy_shape(actor_critic)
    p = next(actor_critic.parameters())
    if shape is None or not (p.is_cuda and p.dtype == torch.float32):
        return None
    return shape_kernel_family(*shape, generic=generic)


def _named_parameters(actor_critic):
    """The MLP's 13 parameters under the member names of solorl_policy_params / solorl_ppo_grads"""
    b, d = actor_critic.base, actor_critic.pi_dist
    return {"critic_w0": b.critic[0].weight, "critic_b0": b.critic[0].bias, "critic_w1": b.critic[2].weight, "critic_b1": b.critic[2].bias,
            "critic_w2": b.critic[4].weight, "critic_b2": b.critic[4].bias, "actor_w0": b.features[0].weight, "actor_b0": b.features[0].bias,
            "actor_w1": b.features[2].weight, "actor_b1": b.features[2].bias, "mean_w": d.mean.weight, "mean_b": d.mean.bias,
            "logstd": d.logstd}


def policy_params(actor_critic, family=TEMPLATED):
    """solorl_policy_params over the module's own parameter storage (PyTorch layout is the kernels' layout: no copies).
    The pointers stay valid as long as the parameters are updated in place (optimizers do).  ``family``: the entry points the calls
    below use with this table (policy_kernel_family)."""
    b, d = actor_critic.base, actor_critic.pi_dist
    P = _native.PolicyParams()
    P.obs_dim, P.hidden, P.act_dim = b.features[0].in_features, b.features[0].out_features, d.mean.out_features
    P.critic_obs_dim = getattr(actor_critic, "critic_obs_dim", None) or 0       # 0: symmetric
    named = _named_parameters(actor_critic)
    for k, t in named.items():
        assert t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
        setattr(P, k, t.data_ptr())
    P._tensors = named            # keeps the storages alive and lets check_params() notice a re-allocated parameter
    assert family in (TEMPLATED, GENERIC)
    P.family = family
    return P


def check_params(P):
    """The kernels read the parameters through raw pointers taken once: a parameter that was re-allocated since (module.to(),
    load_state_dict(assign=True), p.data = ...) would be read from freed memory.  Host-side check, so it guards eager calls and
    graph CAPTURES; a graph replayed after such a change cannot be guarded and must be rebuilt."""
    for k, t in P._tensors.items():
        if getattr(P, k) != t.data_ptr():
            raise RuntimeError("policy parameter %s moved since solorl_policy_params was built; rebuild it (and any HIP graph)" % k)


def _call(params, name, args, critic, both_forms=False):
    """The entry point `name` of the symmetric policy on `args` (what follows the parameters), or, where params.critic_obs_dim is set,
    `name`_critic with the critic's arrays put in: critic = {position in that argument list: tensor}.  The generic family: `name`_w,
    which takes the critic's arrays in the same places, null for a symmetric policy"""
    if params.family == GENERIC:
        name += "_w"
        for i in sorted(critic):
            args.insert(i, C.c_void_p(critic[i].data_ptr() if params.critic_obs_dim else None))
    elif params.critic_obs_dim and not both_forms:         # (both_forms: one templated entry point serves either policy)
        name += "_critic"
        for i in sorted(critic):
            args.insert(i, C.c_void_p(critic[i].data_ptr()))
    _native.check(getattr(_native.lib(), name)(C.byref(params), *args))


def policy_act(params, obs, noise, value_out, action_out, logp_out, critic_obs=None):
    """Policy.act (agents/ppo/policy.py:33-49) in one launch: value_out [N,1], action_out [N,A] = mean + exp(logstd) * noise
    (noise [N,A] standard normal, or None for the deterministic action), logp_out [N,1].  ``critic_obs`` [N, OC]: the critic's rows
    of an asymmetric policy (params.critic_obs_dim = OC), required by one and refused by a symmetric one (solorl_policy_act_critic)."""
    check_params(params)
    n = obs.shape[0]
    dev = obs.device
    for t in (obs, value_out, action_out, logp_out) + (() if noise is None else (noise,)) + (() if critic_obs is None else (critic_obs,)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert obs.shape == (n, params.obs_dim) and action_out.shape == (n, params.act_dim) and value_out.numel() == n and logp_out.numel() == n
    assert (critic_obs is None) == (params.critic_obs_dim == 0), "critic_obs goes with a policy made with critic_obs_dim, and only with one"
    assert critic_obs is None or critic_obs.shape == (n, params.critic_obs_dim)
    with torch.cuda.device(dev):
        _call(params, "solorl_policy_act", [C.c_void_p(obs.data_ptr()), C.c_void_p(0 if noise is None else noise.data_ptr()), n, C.c_void_p(value_out.data_ptr()),
                                            C.c_void_p(action_out.data_ptr()), C.c_void_p(logp_out.data_ptr()), dev.index or 0, _native.stream(dev)],
              {1: critic_obs})


class MiniBatchGrad:
    """One PPO mini-batch step's gradients without autograd, three launches: solorl_ppo_grad_stage1 (gather, forward, losses,
    back-propagation to every layer's pre-activation gradient, written in tiles [row / 32][unit][32]), then solorl_ppo_grad_stage2 (the weight
    gradients G^T X of the six layers over row chunks, and their fixed-order sum written straight into the parameters' .grad --
    views of the flat bucket -- with the log-std gradient and the running loss sums).  Same arithmetic as PPO.update's
    loss.backward() (agents/ppo/ppo.py:46-74) in a different summation order."""
    SLICE = 64                        # mini-batch rows must fill whole wavefronts

    def __init__(self, actor_critic, storage, mini_batch, clip, value_coef, entropy_coef, clipped_value, perm, offset, adv, family=TEMPLATED,
                 diagnostics=False):
        n, m = storage.num_samples, mini_batch
        assert m % self.SLICE == 0, "mini-batch must be a multiple of %d rows" % self.SLICE
        dev = storage.device
        self.ac, self.m = actor_critic, m
        self.P = policy_params(actor_critic, family)
        O, A, H = self.P.obs_dim, self.P.act_dim, 64
        OC = self.OC = self.P.critic_obs_dim          # 0: symmetric
        self.A = A
        flat = lambda x: x.reshape(n, *x.shape[2:])
        B = self.B = _native.PpoBatch()
        self._keep = (flat(storage.obs[:-1]), flat(storage.actions), flat(storage.action_log_probs), adv, flat(storage.value_preds[:-1]),
                      flat(storage.returns[:-1]), perm, offset)
        for k, t in zip(("obs", "actions", "old_logp", "adv", "vpred", "ret", "perm", "offset"), self._keep):
            assert t.is_contiguous() and t.is_cuda
            setattr(B, k, t.data_ptr())
        assert self._keep[0].data_ptr() == storage.obs.data_ptr() and perm.dtype == torch.long and offset.dtype == torch.long
        B.m, B.clipped_value, B.clip, B.value_coef = m, int(bool(clipped_value)), float(clip), float(value_coef)
        # an asymmetric policy: the rollout's critic rows, gathered like obs, and the critic's own xt0 (stage 1 then writes the actor's rows to xt0)
        self.cobs = self.cxt0 = None
        if OC:
            self.cobs = flat(storage.critic_obs[:-1])
            assert self.cobs.is_contiguous() and self.cobs.data_ptr() == storage.critic_obs.data_ptr() and self.cobs.shape[1] == OC
            self.cxt0 = torch.zeros(OC, m, device=dev)

        z = lambda u: torch.zeros(u, m, device=dev)
        xt = z                                # (activations [units][m]; the bias gradients are row sums of g, no row of ones)
        self.buf = dict(xt0=xt(O), c_xt1=xt(H), c_xt2=xt(H), c_g1=z(H), c_g2=z(H), c_gh=z(1), a_xt1=xt(H), a_xt2=xt(H), a_g1=z(H), a_g2=z(H),
                        a_gh=z(A), partials=torch.zeros((m + 31) // 32, 3 + A, device=dev))
        W = self.W = _native.PpoStage1()
        for k, t in self.buf.items():
            setattr(W, k, t.data_ptr())
        # diagnostics: stage 1 through solorl_ppo_grad_stage1_kl, which also leaves per 32 rows (sum of the KL estimate, clipped rows)
        self.diag = torch.zeros(m // 32, 2, device=dev) if diagnostics else None
        self.psum = torch.zeros(3 + A, device=dev)          # running sums of the partials over the steps of an update
        self.ent = torch.zeros(1, device=dev)               # running sum of sum_a logstd_a
        L = _native.lib()
        self.scratch = torch.zeros(L.solorl_ppo_scratch_count2(O, OC or O, A, m), device=dev)
        G = self.G = _native.PpoGrads()
        for k, prm in _named_parameters(actor_critic).items():
            g = prm.grad
            assert g is not None and g.is_contiguous() and g.shape == prm.shape, "parameters need dense .grad tensors (FlatGradBucket)"
            setattr(G, k, g.data_ptr())
        G.loss_sums, G.logstd_sum, G.scratch, G.entropy_coef = self.psum.data_ptr(), self.ent.data_ptr(), self.scratch.data_ptr(), float(entropy_coef)

    def __call__(self):
        check_params(self.P)
        dev = self.psum.device
        with torch.cuda.device(dev):
            st = _native.stream(dev)
            if self.diag is not None:
                crit = lambda t: C.c_void_p(t.data_ptr() if self.OC else None)
                _native.check(_native.lib().solorl_ppo_grad_stage1_kl(C.byref(self.P), C.byref(self.B), crit(self.cobs), C.byref(self.W), crit(self.cxt0),
                                                                      C.c_void_p(self.diag.data_ptr()), int(self.P.family == GENERIC), dev.index or 0, st))
            else:
                _call(self.P, "solorl_ppo_grad_stage1", [C.byref(self.B), C.byref(self.W), dev.index or 0, st], {1: self.cobs, 3: self.cxt0})
            _call(self.P, "solorl_ppo_grad_stage2", [C.byref(self.W), self.m, C.byref(self.G), dev.index or 0, st], {1: self.cxt0})

    def losses(self, steps):
        """(value loss, action loss, entropy) averaged over `steps` mini-batch steps since reset()."""
        v, a = (self.psum[:2] / (self.m * max(steps, 1))).tolist()
        e = 0.5 + _HALF_LOG_2PI + self.ent.item() / (self.A * max(steps, 1))
        return v, a, e

    def reset(self):
        self.psum.zero_(); self.ent.zero_()


class ClipAdam:
    """clip_grad_norm_ + Adam (torch.optim.Adam's arithmetic, agents/ppo/ppo.py:32,75-77) for the MLP policy in ONE launch
    (solorl_ppo_clip_adam) instead of nine; also advances the mini-batch cursor.  The learning rate is read from `lr`, a device
    tensor (the linear schedule rewrites it between updates); moments and the step count live here."""

    def __init__(self, mini_batch_grad, lr, max_grad_norm, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, offset=None, offset_increment=0, grad_scale=1.0,
                 kl_control=None):
        mb = mini_batch_grad
        dev = mb.psum.device
        L = _native.lib()
        n = L.solorl_ppo_grad_count2(mb.P.obs_dim, mb.P.critic_obs_dim or mb.P.obs_dim, mb.P.act_dim) + mb.P.act_dim
        assert n == sum(p.numel() for p in mb.ac.parameters())
        self.P, self.G, self.dev = mb.P, mb.G, dev
        self.exp_avg, self.exp_avg_sq = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.step = torch.zeros(1, device=dev)
        assert torch.is_tensor(lr) and lr.is_cuda and lr.dtype == torch.float32
        self.lr = lr
        S = self.S = _native.AdamState()
        S.exp_avg, S.exp_avg_sq, S.step, S.lr = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step.data_ptr(), lr.data_ptr()
        S.offset, S.offset_increment = (offset.data_ptr() if offset is not None else 0), int(offset_increment)
        S.beta1, S.beta2, S.eps, S.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
        S.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        S.grad_scale = float(grad_scale)     # 1 / world: the gradients arrive SUMMED over the ranks (FlatGradBucket.all_reduce_sum)
        self._offset = offset
        # kl_control = dict(desired_kl, target_kl, lr_factor, lr_bounds, log_capacity), each optional: the step through
        # solorl_ppo_clip_adam_kl, which reads the mini-batch's KL from the diagnostics of `mini_batch_grad` and adapts lr / stops on it
        # (include/solorl.h has the rule).  An empty dict only measures: state and log are filled, nothing is decided.
        self.K = None
        if kl_control is not None:
            assert mb.diag is not None, "kl_control needs MiniBatchGrad(..., diagnostics=True)"
            unknown = set(kl_control) - {"desired_kl", "target_kl", "lr_factor", "lr_bounds", "log_capacity"}
            assert not unknown, "unknown kl_control keys %s" % sorted(unknown)
            cap = int(kl_control.get("log_capacity", 0))
            self.kl_state = torch.zeros(8, device=dev)
            self.kl_log = torch.zeros(cap, 4, device=dev) if cap > 0 else None
            lo, hi = kl_control.get("lr_bounds", (1e-5, 1e-2))
            K = self.K = _native.KlControl()
            K.diag, K.m, K.lr, K.state = mb.diag.data_ptr(), mb.m, lr.data_ptr(), self.kl_state.data_ptr()
            K.desired_kl, K.target_kl = float(kl_control.get("desired_kl") or 0.0), float(kl_control.get("target_kl") or 0.0)
            K.lr_factor, K.lr_min, K.lr_max = float(kl_control.get("lr_factor", 1.5)), float(lo), float(hi)
            K.log, K.log_capacity = (self.kl_log.data_ptr() if cap > 0 else None), cap
            self._keep_diag = mb.diag

    def __call__(self):
        with torch.cuda.device(self.dev):
            if self.K is not None:
                _native.check(_native.lib().solorl_ppo_clip_adam_kl(C.byref(self.P), C.byref(self.G), C.byref(self.S), C.byref(self.K),
                                                                    int(self.P.family == GENERIC), self.dev.index or 0, _native.stream(self.dev)))
                return
            _call(self.P, "solorl_ppo_clip_adam", [C.byref(self.G), C.byref(self.S), self.dev.index or 0, _native.stream(self.dev)], {}, both_forms=True)

    def zero_state(self):
        self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.step.zero_()

    def clear_kl(self):
        """the controller's state (the stopped flag with it) and log, at the start of an update"""
        self.kl_state.zero_()
        if self.kl_log is not None:
            self.kl_log.zero_()

    def kl_diagnostics(self):
        """what the controller saw since clear_kl(): means over the steps seen, the lr last used, the step counts"""
        seen, applied, skl, scf, stopped, _kl, _cf, lr = self.kl_state.tolist()
        n = max(seen, 1.0)
        return dict(approx_kl=skl / n, clip_fraction=scf / n, lr=lr, steps=int(seen), steps_applied=int(applied), stopped=bool(stopped))
