"""On-device rollout storage -- surface of the reference's OPBuffer (agents/ppo/storage.py:5-71):
tensors obs[T+1,N,O], rewards/value_preds/returns/action_log_probs[.,N,1], actions[T,N,A],
masks[T+1,N,1]; append / reset / compute_returns (GAE and plain discounted) / batch_generator.
With ``critic_obs_dim=OC`` also critic_obs[T+1,N,OC], the rows an asymmetric policy's critic reads (policy.py), carried like obs.
With ``bootstrap_timeouts=True`` also timeouts[T,N,1] (uint8), the engine's info["timeout"] of every step: compute_returns then does
not treat an episode the time limit ended as a fall (include/solorl.h solorl_compute_returns_tl).

Everything lives on the rollout device, so a 4096-env x 400-step buffer (~0.55 GB for Solo12
pointGoal) never crosses PCIe; mini-batches are gathered with one index_select per tensor."""
import torch


class RolloutStorage:
    def __init__(self, num_steps, num_agents, obs_shape, action_dim, device, critic_obs_dim=None, bootstrap_timeouts=False):
        z = lambda *s: torch.zeros(*s, device=device)
        self.obs = z(num_steps + 1, num_agents, *obs_shape)
        self.critic_obs = None if critic_obs_dim is None else z(num_steps + 1, num_agents, int(critic_obs_dim))
        self.rewards = z(num_steps, num_agents, 1)
        self.value_preds = z(num_steps + 1, num_agents, 1)
        self.returns = z(num_steps + 1, num_agents, 1)
        self.action_log_probs = z(num_steps, num_agents, 1)
        self.actions = z(num_steps, num_agents, action_dim)
        self.masks = torch.ones(num_steps + 1, num_agents, 1, device=device)
        self.timeouts = torch.zeros(num_steps, num_agents, 1, dtype=torch.uint8, device=device) if bootstrap_timeouts else None
        self.num_steps, self.num_agents = num_steps, num_agents
        self.num_samples = num_steps * num_agents
        self.device = device
        self.step = 0

    def append(self, obs, actions, action_log_probs, value_preds, rewards, masks, critic_obs=None, timeouts=None):
        t = self.step
        if (critic_obs is None) != (self.critic_obs is None):
            raise ValueError("critic_obs goes with a storage made with critic_obs_dim, and only with one")
        if (timeouts is None) != (self.timeouts is None):
            raise ValueError("timeouts goes with a storage made with bootstrap_timeouts, and only with one")
        self.obs[t + 1].copy_(obs)
        if critic_obs is not None:
            self.critic_obs[t + 1].copy_(critic_obs)
        self.actions[t].copy_(actions)
        self.action_log_probs[t].copy_(action_log_probs)
        self.value_preds[t].copy_(value_preds)
        self.rewards[t].copy_(rewards)
        self.masks[t + 1].copy_(masks)
        if timeouts is not None:
            self.timeouts[t].copy_(timeouts.reshape(self.timeouts[t].shape))
        self.step = (t + 1) % self.num_steps

    def reset(self):
        self.obs[0].copy_(self.obs[-1])
        if self.critic_obs is not None:
            self.critic_obs[0].copy_(self.critic_obs[-1])
        self.masks[0].copy_(self.masks[-1])

    @torch.no_grad()
    def compute_returns(self, next_value, use_gae=True, gamma=0.99, gae_lambda=0.95):
        """storage.py:35-55.  GAE: delta_t = r_t + g V_{t+1} m_{t+1} - V_t,
        A_t = delta_t + g l m_{t+1} A_{t+1}, R_t = A_t + V_t;  else R_t = r_t + g m_{t+1} R_{t+1}.
        A storage made with bootstrap_timeouts (include/solorl.h solorl_compute_returns_tl): where m_{t+1} = 0 and timeouts[t] is set,
        V_t with weight 1 stands for V_{t+1} m_{t+1} (for R_{t+1} m_{t+1}): the step the time limit cut off bootstraps from the value
        of the observation its action was taken from.  Every other sample keeps its arithmetic, and its bits."""
        T = self.num_steps
        if self.rewards.is_cuda:      # fused HIP kernel; raises if the engine library is missing
            import ctypes as C
            from .. import _native
            dev = self.rewards.device
            nv = next_value.detach().to(torch.float32).contiguous()
            p = [C.c_void_p(x.data_ptr()) for x in (self.rewards, self.value_preds, self.masks, nv, self.returns)]
            tail = (T, self.num_agents, int(bool(use_gae)), float(gamma), float(gae_lambda), dev.index or 0, _native.stream(dev))
            with torch.cuda.device(dev):
                if self.timeouts is None:
                    _native.check(_native.lib().solorl_compute_returns(*p, *tail))
                else:
                    _native.check(_native.lib().solorl_compute_returns_tl(*p[:3], C.c_void_p(self.timeouts.data_ptr()), *p[3:], *tail))
            return
        v, m = self.value_preds, self.masks
        # the truncated steps, or None: then every expression below is the plain one, and so are its bits
        tl = None if self.timeouts is None else (m[1:] == 0) & (self.timeouts != 0)
        if use_gae:
            v[-1].copy_(next_value)
            if tl is None:
                delta = self.rewards + gamma * v[1:] * m[1:] - v[:-1]       # one fused elementwise pass
            else:                                                         # the same expression on the selected operands
                delta = self.rewards + gamma * torch.where(tl, v[:-1], v[1:]) * m[1:].masked_fill(tl, 1.0) - v[:-1]
            coef = (gamma * gae_lambda) * m[1:]
            adv = torch.zeros_like(next_value)
            for t in range(T - 1, -1, -1):                                # the recurrence itself is sequential in t
                adv = torch.addcmul(delta[t], coef[t], adv)
                self.returns[t] = adv + v[t]
        else:
            self.returns[-1].copy_(next_value)
            gm = gamma * (m[1:] if tl is None else m[1:].masked_fill(tl, 1.0))
            for t in range(T - 1, -1, -1):
                # (a truncated step takes V_t in the carry's place, as the kernel does: nothing of the later returns reaches it)
                nxt = self.returns[t + 1] if tl is None else torch.where(tl[t], v[t], self.returns[t + 1])
                self.returns[t] = torch.addcmul(self.rewards[t], gm[t], nxt)

    def batch_generator(self, advantages, mini_batch_size, generator=None):
        """storage.py:57-71: random mini-batches without replacement, incomplete last batch dropped.  A storage with critic rows yields
        them as an eighth element; one without yields the reference's seven."""
        n = self.num_samples
        perm = torch.randperm(n, device=self.device, generator=generator)
        flat = lambda x: x.reshape(n, *x.shape[2:])
        obs, act, val = flat(self.obs[:-1]), flat(self.actions), flat(self.value_preds[:-1])
        ret, msk, olp, adv = flat(self.returns[:-1]), flat(self.masks[:-1]), flat(self.action_log_probs), advantages.reshape(n, 1)
        for s in range(0, n - mini_batch_size + 1, mini_batch_size):
            idx = perm[s:s + mini_batch_size]
            batch = obs[idx], act[idx], val[idx], ret[idx], msk[idx], olp[idx], adv[idx]
            yield batch if self.critic_obs is None else batch + (flat(self.critic_obs[:-1])[idx],)


OPBuffer = RolloutStorage   # the reference's class name
