"""PPO KL control: the rule that the device applies in solorl_ppo_clip_adam_kl (include/solorl.h has the table) as a pure host
function in the same f32 arithmetic, and the bookkeeping the PyTorch paths of PPO.update share with it.

approx_kl is Schulman's k3 estimator, mean((ratio - 1) - log ratio) -- stable-baselines' approx_kl; it needs nothing the rollout does
not store.  desired_kl drives the learning rate as rsl_rl's "adaptive" schedule does, target_kl ends an update as stable-baselines'
does (at 1.5 x target_kl)."""
import numpy as np

F = np.float32


def kl_rule(kl, lr, stopped=False, desired_kl=None, target_kl=None, lr_factor=1.5, lr_min=1e-5, lr_max=1e-2):
    """One mini-batch step's decision -> (lr to use and to keep, as np.float32; stopped).  In this order:
    1. target_kl > 0 and kl > 1.5 target_kl: stopped (and it stays so);
    2. not stopped and desired_kl > 0: kl > 2 desired_kl: lr = max(lr_min, lr / lr_factor); else kl < desired_kl / 2 and kl > 0:
       lr = min(lr_max, lr * lr_factor).
    A kl that is not finite decides nothing."""
    kl, lr = F(kl), F(lr)
    d, t = F(desired_kl or 0.0), F(target_kl or 0.0)
    finite = bool(np.isfinite(kl))
    stopped = bool(stopped)
    if finite and t > 0 and kl > F(1.5) * t:
        stopped = True
    if not stopped and d > 0:
        if finite and kl > F(2.0) * d:
            lr = max(F(lr_min), F(lr / F(lr_factor)))
        elif finite and kl < d / F(2.0) and kl > 0:
            lr = min(F(lr_max), F(lr * F(lr_factor)))
    return F(lr), stopped


class KlSettings:
    """desired_kl / target_kl / diagnostics as PPO takes them; `on` is False when none is asked for"""

    def __init__(self, desired_kl=None, target_kl=None, diagnostics=False, lr_factor=1.5, lr_bounds=(1e-5, 1e-2)):
        self.desired_kl = float(desired_kl) if desired_kl else None
        self.target_kl = float(target_kl) if target_kl else None
        self.lr_factor, self.lr_bounds = float(lr_factor), (float(lr_bounds[0]), float(lr_bounds[1]))
        if not self.lr_factor > 1.0:
            raise ValueError("lr_factor must be > 1")
        if self.lr_bounds[0] > self.lr_bounds[1]:
            raise ValueError("lr_bounds: the lower bound exceeds the upper")
        self.on = bool(diagnostics or self.desired_kl or self.target_kl)

    def rule(self, kl, lr, stopped):
        return kl_rule(kl, lr, stopped, self.desired_kl, self.target_kl, self.lr_factor, self.lr_bounds[0], self.lr_bounds[1])

    def as_dict(self, log_capacity=0):
        """ClipAdam's kl_control"""
        return dict(desired_kl=self.desired_kl, target_kl=self.target_kl, lr_factor=self.lr_factor, lr_bounds=self.lr_bounds, log_capacity=log_capacity)


def summarize(log, lr):
    """last_diagnostics from a step log [[kl, clip fraction, lr used, applied], ...]; lr: the rate in force when no step was logged"""
    n = len(log)
    applied = int(sum(r[3] for r in log))
    return dict(approx_kl=float(sum(r[0] for r in log)) / max(n, 1), clip_fraction=float(sum(r[1] for r in log)) / max(n, 1),
                lr=float(log[-1][2]) if n else float(lr), steps=n, steps_applied=applied, stopped=applied < n)
