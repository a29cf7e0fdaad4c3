"""HIP-graph capture of the two launch-bound loops of PPO training on a GPU (PyTorch's CUDAGraph API is
hipGraph on ROCm).

At 4096 envs the engine's step kernel takes ~0.2 ms, a policy forward ~10 small kernels and a PPO
mini-batch step (gather, forward, losses, backward, clip, Adam) ~100 kernels of a few microseconds each:
run eagerly, both loops are bound by launch latency and Python, not by the GPU.  Captured once and
replayed, a whole T-step rollout is ONE graph launch and every mini-batch step one (two with a
gradient all-reduce between them when world > 1).

  GraphedRollout  act -> solorl_step (the C-ABI launch is captured like any other kernel: it is enqueued on
                  torch's capturing stream and never synchronises) -> storage.append, T times
                  (opt-in, chunk = K: windows of K closed-loop steps, one solorl_rollout launch each)
  GraphedPPO      PPO.update with identical arithmetic (agents/ppo/ppo.py:34-89); mini-batch indices are
                  read on the device from a permutation buffer at a device-side offset, so a replay needs
                  no host-side argument

Both fall back to nothing: they are only constructed for CUDA devices; train() uses them unless
--no-hip-graphs is given."""
import os

import torch
import torch.nn as nn

from . import dist as D
from .fused import TEMPLATED, ClipAdam, MiniBatchGrad, fused_ppo_loss, policy_act, policy_kernel_family, policy_params
from .ppo import PPO


def _kernels_enabled():
    """SOLORL_PPO_KERNELS=0 keeps the rollout's act and the mini-batch step on their PyTorch paths (A/B runs)."""
    return os.environ.get("SOLORL_PPO_KERNELS", "1") != "0"


def _generic_switch():
    """SOLORL_POLICY_GENERIC: 0 or unset, the policy kernels built per shape or the PyTorch path; 1, the width-generic kernels for the
    shapes the per-shape family does not build; 2, the width-generic kernels for every shape they take (A/B runs)."""
    return int(os.environ.get("SOLORL_POLICY_GENERIC", "0") or 0)


def _policy_family(actor_critic):
    """The kernel family both loops run this policy on (fused.policy_kernel_family), None = the PyTorch path"""
    return policy_kernel_family(actor_critic, _generic_switch()) if _kernels_enabled() else None


def capture_kwargs():
    """With a process group up, its watchdog thread issues HIP calls of its own; a capture in the default "global" error mode
    would be invalidated by them.  Thread-local mode confines the capture's checks to the capturing thread."""
    return {"capture_error_mode": "thread_local"} if D.world() > 1 else {}


def _side_stream_warmup(fn, iters=3):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(iters):
            fn()
    torch.cuda.current_stream().wait_stream(s)


def probe_captured_allreduce(dev, numel, replays=8, time_it=False):
    """Does an all-reduce(sum) of `numel` floats -- the real bucket size -- run at every REPLAY of a captured graph?  (A collective that
    ran at capture time only would leave stale data.)  Returns (ok, seconds per replay or None); ok is the same on every rank.

    Protocol (a rank whose capture raised must not sit in a different collective than its peers): every step that can
    differ between ranks is followed by an EAGER MIN all-reduce of a flag that every rank reaches --
      1. eager all-reduce (communicator set up outside any capture)
      2. capture, in a try block                       -> agree: did EVERY rank capture?  no: return False everywhere, nobody replays
      3. `replays` replays with different inputs, each result checked against the closed form   -> agree on the outcome."""
    import time
    import torch.distributed as dist
    w, r = D.world(), D.rank()

    def agree(flag):
        t = torch.tensor([1 if flag else 0], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    probe = torch.zeros(int(numel), device=dev)
    dist.all_reduce(probe)
    torch.cuda.synchronize()
    g, captured = None, True
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, **capture_kwargs()):
            dist.all_reduce(probe, op=dist.ReduceOp.SUM)
    except Exception:
        captured = False
    if not agree(captured):
        return False, None
    ok = True
    for k in range(1, replays + 1):
        probe.fill_(float(k * (r + 1)))
        g.replay()
        torch.cuda.synchronize()
        ok = ok and bool((probe == float(k * w * (w + 1) // 2)).all().item())
    ok = agree(ok)
    sec = None
    if ok and time_it:
        probe.zero_()                         # (sums of zeros: the timing loop cannot overflow)
        torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        for _ in range(50):
            g.replay()
        torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / 50
    return ok, sec


class GraphedRollout:
    """One graph = num_steps x (policy.act, env.step, storage.append).  Episode statistics need nothing here: the step
    kernel accumulates them on the device (include/solorl.h `ep_stats`), replayed or not."""

    def __init__(self, envs, actor_critic, storage, num_steps, chunk=None):
        self.envs, self.ac, self.storage, self.T = envs, actor_critic, storage, num_steps
        # chunk = K > 0: the rollout as ceil(T / K) windows of K closed-loop steps, ONE launch each (solorl_rollout: no wavefront waits
        # for another between the steps of a window), where the handle supports it.  Default SOLORL_ROLLOUT_CHUNK, 0 = one launch per step.
        self.chunk = int(os.environ.get("SOLORL_ROLLOUT_CHUNK", "0")) if chunk is None else int(chunk)
        self.windows = None          # the window lengths the captured body used (None: not chunked)
        self.graph = None

    def _body(self):
        st = self.storage
        assert st.step == 0, "graphed rollouts start at storage step 0"
        # the arithmetic of train.rollout() with every result written where it is stored: the policy's outputs and the engine's
        # observations / rewards / done flags go straight into storage-side rows (the C ABI takes caller-owned pointers) -- two
        # launches per step (act, env step) instead of 35, and launches are what a step costs besides the env kernel
        # an asymmetric policy (storage with critic rows): the critic reads st.critic_obs[t], which the env writes beside st.obs[t + 1]:
        # one policy launch per step (solorl_policy_act_critic where the shape is built, else act_into) plus the env's launches
        asym = getattr(st, "critic_obs", None) is not None
        # a storage made with bootstrap_timeouts: every step launch writes its timeout flags into the storage's row by itself (the info
        # block it is handed points there) -- no launch more, in any branch
        tout = getattr(st, "timeouts", None)
        family = _policy_family(self.ac)
        fused = family is not None
        if fused:                            # one launch for the whole of Policy.act (csrc/solorl_ppo.hip)
            self._pp = policy_params(self.ac, family)
        # the normal draws of all T steps and masks = 1 - done of all T steps are one launch each per rollout, not per step
        noise = torch.randn_like(st.actions) if fused else None
        done = torch.empty(self.T, st.num_agents, dtype=torch.uint8, device=st.device)
        # ONE launch per rollout step where the engine supports it (solorl_step_act: each wavefront of the step kernel evaluates the policy
        # on the observations it has just produced, in the time it would otherwise idle until the slowest wavefront ends); the first
        # step's action still needs its own policy launch.  SOLORL_STEP_ACT=0 keeps the two-launch form (A/B runs).
        # (the step kernel's policy tail is built per shape: the width-generic family always acts in a launch of its own)
        self.step_act = bool(family == TEMPLATED and os.environ.get("SOLORL_STEP_ACT", "1") != "0" and hasattr(self.envs, "step_act_supported")
                             and self.envs.step_act_supported(self._pp))
        if family == TEMPLATED and self.chunk > 0 and hasattr(self.envs, "rollout_supported") and self.envs.rollout_supported(self._pp):
            # row 0's action from its own policy launch, then windows of K steps straight into storage rows; every window but the last
            # also evaluates the policy after its last step (row t0 + K: the next window's first action)
            policy_act(self._pp, st.obs[0], noise[0], st.value_preds[0], st.actions[0], st.action_log_probs[0])
            self.windows = []
            for t0 in range(0, self.T, self.chunk):
                K = min(self.chunk, self.T - t0)
                pal = 1 if t0 + K < self.T else 0
                R = K + pal
                self.envs.rollout_inplace(st.actions[t0:t0 + R], self._pp, noise[t0:t0 + R], st.value_preds[t0:t0 + R], st.action_log_probs[t0:t0 + R],
                                          obs_out=st.obs[t0 + 1:t0 + 1 + K], rew_out=st.rewards[t0:t0 + K], done_out=done[t0:t0 + K], policy_after_last=pal,
                                          timeout_out=None if tout is None else tout[t0:t0 + K])
                self.windows.append(K)
            torch.sub(torch.ones((), device=st.device), done, out=st.masks[1:].view(self.T, st.num_agents))
            return
        for t in range(self.T):
            to_t = None if tout is None else tout[t]
            if self.step_act:
                if t == 0:
                    policy_act(self._pp, st.obs[0], noise[0], st.value_preds[0], st.actions[0], st.action_log_probs[0])
                if t + 1 < self.T:
                    self.envs.step_act_inplace(st.actions[t], self._pp, noise[t + 1], st.value_preds[t + 1], st.actions[t + 1], st.action_log_probs[t + 1],
                                               obs_out=st.obs[t + 1], rew_out=st.rewards[t], done_out=done[t], timeout_out=to_t)
                else:
                    self.envs.step_inplace(st.actions[t], obs_out=st.obs[t + 1], rew_out=st.rewards[t], done_out=done[t], timeout_out=to_t)
                continue
            if fused:
                policy_act(self._pp, st.obs[t], noise[t], st.value_preds[t], st.actions[t], st.action_log_probs[t],
                           critic_obs=st.critic_obs[t] if asym else None)
            elif asym:
                self.ac.act_into(st.obs[t], st.value_preds[t], st.actions[t], st.action_log_probs[t], critic_inputs=st.critic_obs[t])
            else:
                self.ac.act_into(st.obs[t], st.value_preds[t], st.actions[t], st.action_log_probs[t])
            if asym:
                self.envs.step_inplace(st.actions[t], obs_out=st.obs[t + 1], rew_out=st.rewards[t], done_out=done[t], critic_obs_out=st.critic_obs[t + 1], timeout_out=to_t)
                continue
            self.envs.step_inplace(st.actions[t], obs_out=st.obs[t + 1], rew_out=st.rewards[t], done_out=done[t], timeout_out=to_t)
        torch.sub(torch.ones((), device=st.device), done, out=st.masks[1:].view(self.T, st.num_agents))

    def _capturable(self):
        # contact-count sorting (opt-in, SOLORL_SORT=1) ping-pongs two state buffers on the host side of
        # solorl_step: a captured sequence is only self-consistent over an even number of steps.  Asked of the handle (the engine
        # latches the switch at solorl_create); an env without the engine's properties does not sort
        sort = hasattr(self.envs, "get_property") and self.envs.get_property("sort") != 0
        return not sort or self.T % 2 == 0

    def __call__(self):
        if not self._capturable():
            from .train import rollout
            return rollout(self.envs, self.ac, self.storage, self.T)
        if self.graph is None:
            # no warm-up replay of the body: the env must not be stepped twice.  Everything the body allocates
            # is allocated inside the capture (private pool); cuBLAS/hipBLASLt workspaces were created by the
            # eager policy calls that precede the first rollout (train(): reset + get_value warm-up).
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, **capture_kwargs()):
                self._body()
            self.graph = g
        self.graph.replay()


class GraphedPPO(PPO):
    """PPO with the mini-batch step captured.  Adam runs in capturable mode with the learning rate held in a
    device tensor (update_linear_schedule fills it), otherwise the arithmetic is PPO.update's."""

    def __init__(self, actor_critic, clip_param, ppo_epoch, mini_batch_size, value_loss_coef, entropy_coef, lr=None,
                 l2_coef=0.0, max_grad_norm=None, use_clipped_value_loss=True, fused_loss=True, fused_mlp=True, desired_kl=None, target_kl=None,
                 diagnostics=False, lr_factor=1.5, lr_bounds=(1e-5, 1e-2)):
        super().__init__(actor_critic, clip_param, ppo_epoch, mini_batch_size, value_loss_coef, entropy_coef, lr=lr,
                         l2_coef=l2_coef, max_grad_norm=max_grad_norm, use_clipped_value_loss=use_clipped_value_loss, desired_kl=desired_kl,
                         target_kl=target_kl, diagnostics=diagnostics, lr_factor=lr_factor, lr_bounds=lr_bounds)
        self.fused_loss = fused_loss
        # hand-written mini-batch kernel (csrc/solorl_ppo.hip) where it is built for this policy's shape; otherwise autograd
        self._family = _policy_family(actor_critic) if fused_mlp else None
        self.fused_mlp = self._family is not None
        dev = next(actor_critic.parameters()).device
        # (fused: one multi-tensor launch per optimizer step instead of a dozen -- a captured mini-batch step is ~100 launches of a
        # few microseconds each, so launches are what it costs)
        self.optimizer = torch.optim.Adam(actor_critic.parameters(), lr=torch.tensor(float(lr), device=dev),
                                          weight_decay=l2_coef, capturable=True, fused=True)
        self._built_for = None

    # ---- capture
    def _build(self, storage):
        dev = storage.device
        n, m = storage.num_samples, self.mini_batch_size
        flat = lambda x: x.reshape(n, *x.shape[2:])
        self._src = (flat(storage.obs[:-1]), flat(storage.actions), flat(storage.value_preds[:-1]), flat(storage.returns[:-1]),
                     flat(storage.action_log_probs))
        assert all(s.data_ptr() == b.data_ptr() for s, b in zip(self._src, (storage.obs, storage.actions, storage.value_preds,
                                                                            storage.returns, storage.action_log_probs)))
        # the critic's rows of an asymmetric policy, gathered like the actor's
        self._csrc = flat(storage.critic_obs[:-1]) if getattr(storage, "critic_obs", None) is not None else None
        self._adv = torch.zeros(n, 1, device=dev)
        self._perm = torch.zeros(n, dtype=torch.long, device=dev)
        self._off = torch.zeros((), dtype=torch.long, device=dev)
        self._ar = torch.arange(m, device=dev)
        self._stats = torch.zeros(3, device=dev)
        clip = self.clip_param
        kl = self.kl                          # KL control (kl_control.py); kl.on False: nothing below is allocated or called differently
        kl_steps = self.ppo_epoch * (n // m)  # mini-batch steps of an update = rows of the step log
        kw = dict(diagnostics=True) if kl.on else {}
        self._mb = None
        if self.fused_mlp and m % MiniBatchGrad.SLICE == 0:
            self._mb = MiniBatchGrad(self.actor_critic, storage, m, clip, self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss,
                                     self._perm, self._off, self._adv, family=self._family, **kw)
        self._kl_state = self._kl_log = None
        if kl.on and self._mb is None:
            # the autograd path: the rule as torch ops on the capturable Adam's lr tensor.  That optimizer cannot skip a step
            if kl.target_kl:
                raise NotImplementedError("target_kl needs the mini-batch kernels (a policy shape they are built for, or --generic-policy-kernels) "
                                          "or the eager update (--no-hip-graphs): the captured PyTorch optimizer cannot skip a step")
            t32 = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
            d = kl.desired_kl or 0.0
            self._kl_state, self._kl_log = torch.zeros(8, device=dev), torch.zeros(max(kl_steps, 1), 4, device=dev)
            self._kl_c = dict(f=t32(kl.lr_factor), lr_min=t32(kl.lr_bounds[0]), lr_max=t32(kl.lr_bounds[1]), hi=t32(d) * 2.0, lo=t32(d) / 2.0,
                              one=t32(1.0))

        def kl_ops(ratio, logp, old_lp_b):
            with torch.no_grad():
                c, st, lr_t = self._kl_c, self._kl_state, self.optimizer.param_groups[0]["lr"]
                k = ((ratio - 1.0) - (logp - old_lp_b)).mean()
                cf = ((ratio < 1.0 - clip) | (ratio > 1.0 + clip)).float().mean()
                if kl.desired_kl:
                    fin = torch.isfinite(k)
                    shrink, grow = fin & (k > c["hi"]), fin & (k < c["lo"]) & (k > 0)
                    lr_t.copy_(torch.where(shrink, torch.maximum(c["lr_min"], lr_t / c["f"]),           # (a tensor divisor: a true division)
                                           torch.where(grow, torch.minimum(c["lr_max"], lr_t * c["f"]), lr_t)))
                row = torch.stack([k, cf, lr_t.reshape(()), c["one"]])
                self._kl_log.index_copy_(0, st[0:1].long().clamp(max=self._kl_log.shape[0] - 1), row.unsqueeze(0))
                st[0:4] += torch.stack([c["one"], c["one"], k, cf])
                st[5:8] = row[:3]

        self._ca = None
        if self._mb is not None:             # norm clip + Adam + cursor in one launch; lr stays the optimizer's device tensor
            g0 = self.optimizer.param_groups[0]
            self._ca = ClipAdam(self._mb, g0["lr"], self.max_grad_norm, weight_decay=g0["weight_decay"], betas=g0["betas"], eps=g0["eps"],
                                offset=self._off, offset_increment=m, **(dict(kl_control=kl.as_dict(log_capacity=kl_steps)) if kl.on else {}))

        def fwd_bwd():
            if self._mb is not None:     # three launches: gather + forward + losses + back-propagation; weight gradients; their sum
                self._mb()
                return
            idx = self._perm.index_select(0, self._ar + self._off)
            self._off += m
            obs_b, act_b, vpred_b, ret_b, old_lp_b = (s.index_select(0, idx) for s in self._src)
            adv_b = self._adv.index_select(0, idx)
            critic = {} if self._csrc is None else {"critic_inputs": self._csrc.index_select(0, idx)}
            if self.fused_loss and not kl.on:       # one HIP launch for log-prob, both losses and their head gradients (ppo/fused.py)
                values, mean, logstd = self.actor_critic.heads(obs_b, **critic)
                loss, value_loss, action_loss, entropy = fused_ppo_loss(mean, logstd, values, act_b, old_lp_b, adv_b, vpred_b, ret_b, clip,
                                                                        self.value_loss_coef, self.entropy_coef, self.use_clipped_value_loss)
            else:
                values, logp, entropy = self.actor_critic.evaluate_actions(obs_b, act_b, **critic)
                ratio = torch.exp(logp - old_lp_b)
                if kl.on:             # (these expressions have logp, the fused loss does not)
                    kl_ops(ratio, logp, old_lp_b)
                action_loss = -torch.min(ratio * adv_b, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_b).mean()
                if self.use_clipped_value_loss:
                    v_clipped = vpred_b + (values - vpred_b).clamp(-clip, clip)
                    value_loss = 0.5 * torch.max((values - ret_b).pow(2), (v_clipped - ret_b).pow(2)).mean()
                else:
                    value_loss = 0.5 * (ret_b - values).pow(2).mean()
                loss = value_loss * self.value_loss_coef + action_loss - entropy * self.entropy_coef
            self.bucket.zero()
            loss.backward()
            self._stats += torch.stack([value_loss.detach(), action_loss.detach(), entropy.detach()])

        def opt_step():
            if self._ca is not None:
                self._ca()
                return
            if self.max_grad_norm is not None:
                # clip_grad_norm_ (agents/ppo/ppo.py:75-76) on the flat bucket every .grad is a view of: the 2-norm of the
                # per-tensor norms is the norm of the concatenation
                flat = self.bucket.flat
                flat.mul_((self.max_grad_norm / (flat.norm() + 1e-6)).clamp(max=1.0))
            self.optimizer.step()

        # warm-up on a side stream (allocator, autograd and optimizer state), then put everything back
        params = [p for p in self.actor_critic.parameters()]
        saved = [p.detach().clone() for p in params]
        lr_saved = self.optimizer.param_groups[0]["lr"].detach().clone()     # (the warm-up steps may adapt it)
        self._perm.copy_(torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(0)))   # (own generator: the
                                                                                   # global RNG stream stays the eager path's)
        def warm():
            self._off.zero_()
            fwd_bwd()
            opt_step()
        _side_stream_warmup(warm)
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.copy_(s)
            for st in self.optimizer.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            if self._ca is not None:
                self._ca.zero_state()
            self.optimizer.param_groups[0]["lr"].copy_(lr_saved)
        self._kl_clear()
        self._stats.zero_(); self._off.zero_()
        if self._mb is not None:
            self._mb.reset()
        # world > 1: one flat-bucket all-reduce per optimizer step, between the gradients and the clip.  Default: the
        # SPLIT form -- gradients graph -> eager all-reduce -> optimizer graph (clip + Adam with grad_scale = 1 / world in one launch).
        # SOLORL_CAPTURE_ALLREDUCE=1 with the nccl (= RCCL) backend captures the collective with the rest, so that a mini-batch step is
        # ONE graph replay; a probe graph of the real bucket size first checks on every rank that a captured all-reduce really runs
        # at replay (probe_captured_allreduce).  Opt-in because it has never run on two GPUs.
        w = D.world()
        self._split = False
        if w > 1:
            self._split = not self._collective_is_capturable(dev)
        self.allreduce_in_graph = w > 1 and not self._split
        if self._ca is not None:
            self._ca.S.grad_scale = 1.0 / w          # the bucket arrives SUMMED (all_reduce_sum); the scale is fused into the step
        reduce_ = self.bucket.all_reduce_sum if self._ca is not None else self.bucket.all_reduce_mean
        self._reduce = reduce_
        pool = torch.cuda.graph_pool_handle()
        self._g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g1, pool=pool, **capture_kwargs()):
            fwd_bwd()
            if not self._split:
                if w > 1:
                    reduce_()
                opt_step()
        if self._split:                       # the all-reduce of the flat bucket runs between two graphs
            self._g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._g2, pool=pool, **capture_kwargs()):
                opt_step()
        with torch.no_grad():                 # capture does not execute, but be explicit about the state we start from
            self._stats.zero_(); self._off.zero_()
        self._built_for = (id(storage), n, m)

    def _kl_clear(self):
        if self._ca is not None and self._ca.K is not None:
            self._ca.clear_kl()
        if self._kl_state is not None:
            self._kl_state.zero_(); self._kl_log.zero_()

    def _collective_is_capturable(self, dev):
        """Whether the bucket all-reduce goes INSIDE the captured mini-batch step.  Opt-in (SOLORL_CAPTURE_ALLREDUCE=1) until a real
        multi-GPU run has exercised it: no box of this project has had two GPUs, so the split form (graph -> eager all-reduce -> graph)
        stays the default and `allreduce_in_graph` is recorded with every result."""
        want = D.backend() == "nccl" and os.environ.get("SOLORL_CAPTURE_ALLREDUCE", "0") == "1" and os.environ.get("SOLORL_SPLIT_ALLREDUCE", "0") == "0"
        if not want:
            return False
        ok, _ = probe_captured_allreduce(dev, self.bucket.flat.numel())
        return ok

    def update(self, storage):
        if not storage.rewards.is_cuda:
            return super().update(storage)
        if self._built_for != (id(storage), storage.num_samples, self.mini_batch_size):
            self._build(storage)
        n, m = storage.num_samples, self.mini_batch_size
        adv = storage.returns[:-1] - storage.value_preds[:-1]
        mean, std = D.global_mean_std(adv, unbiased=True)
        self._adv.copy_(((adv - mean) / (std + 1e-5)).reshape(n, 1))
        self._stats.zero_()
        if self._mb is not None:
            self._mb.reset()
        if self.kl.on:
            self._kl_clear()
        n_updates = 0
        for _ in range(self.ppo_epoch):
            if self.kl.target_kl and self._ca.kl_state[4].item() != 0.0:     # stopped: what is left would be replays that apply nothing
                break
            self._perm.copy_(torch.randperm(n, device=storage.device))
            self._off.zero_()
            for _s in range(0, n - m + 1, m):
                self._g1.replay()
                if self._split:
                    self._reduce()
                    self._g2.replay()
                n_updates += 1
        if self.kl.on:
            state, log = (self._ca.kl_state, self._ca.kl_log) if self._mb is not None else (self._kl_state, self._kl_log)
            seen, applied, skl, scf, stopped, _k, _c, lr = state.tolist()
            self.last_diagnostics = dict(approx_kl=skl / max(seen, 1.0), clip_fraction=scf / max(seen, 1.0), lr=lr, steps=int(seen),
                                         steps_applied=int(applied), stopped=bool(stopped))
            self.last_step_log = log[:int(seen)].cpu()
        if self._mb is not None:
            return self._mb.losses(n_updates)
        v, a, e = (self._stats / max(n_updates, 1)).tolist()
        return v, a, e
