"""Gym-style vec-env surface over the HIP engine -- the drop-in for the reference's
``make_vec_envs`` -> ``PyTorchEnvWrapper(VecNormalize(VecEnvWrapper(...)))`` stack
(agents/ppo/envs.py:14-30, :183-222).  Same attribute names, argument meaning and error behaviour:

  reset() -> Tensor[N, O] f32                                  (envs.py:198-200)
  step(actions Tensor[N, A]) -> (obs[N,O], reward[N,1], done[N] f32, infos)   (envs.py:189-196)
  step_n(actions Tensor[K, N, A]) -> (obs[K,N,O], reward[K,N,1], done[K,N] f32, infos)  (K steps, one launch: no reference counterpart)
  get_observation(), increment_curriculum(), close(), observation_space, action_space, nenvs
  ob_rms, ret_rms, training, train(), eval(): the reference's VecNormalize (agents/running_mean_std.py:73-127) when make_vec_envs is given
      norm_obs / norm_ret -- running statistics on the device (normalize.py, include/solorl.h solorl_normalize_obs / solorl_normalize_rewards)
  get_states(mask) -> StateBatch, set_states(states, mask, fields), reset_masked(mask) -> obs, push(dv, mask)   (the whole batch's state as
      one device array, include/solorl.h solorl_get_states ...: no reference counterpart)
  set_perturbation(interval, max_lin_vel, max_ang_vel), perturb(), last_kick, perturbation_state()   (random base kicks drawn and applied on
      the device, in front of every step launch while set: include/solorl.h solorl_set_perturbation / solorl_perturb)
  get_kinematics(mask) -> KinBatch   (link poses, support points of the collision primitives with velocity and normal force, centre of
      mass, energy, momentum of every env: include/solorl.h solorl_kinematics, kinematics.py)
  get_dynamics(mask) -> DynBatch   (joint-space mass matrix, bias and gravity forces, foot Jacobians with their Jdot v of every env:
      include/solorl.h solorl_dynamics, dyn_tensors.py)
  set_reward_shaping(weights, **params), last_shaping_terms, shaping_stats()   (sixteen shaped reward terms -- foot slip, clearance, contact
      force and air time, action rate, joint acceleration, power, command tracking ... -- added to every step's reward by one launch behind
      the step launch while set: include/solorl.h solorl_shape_reward, shaping.py)
  set_obs_noise(scales), set_actuation(delay, gain_range), last_applied_actions   (uniform sensor noise on every observation row the
      engine writes, and actuation latency with a per-joint motor gain error on every action row it reads, drawn on the device per env:
      include/solorl.h solorl_obs_noise / solorl_actuate, channel.py)
  SoloVecEnv(..., commands=dict), set_command_ranges(**ranges), last_commands, engine_obs_dim   (per-env velocity commands drawn from
      ranges and resampled on the device, appended to every observation row as three words and tracked by the shaped reward's two
      tracking terms: include/solorl.h solorl_commands / solorl_shape_reward_cmd, command.py)
  set_termination(**rules), last_termination, termination_stats()   (early termination rules -- base height, tilt, contact of chosen
      primitives, joint limits -- checked on the state after every step by one launch, the envs they end reset on the device:
      include/solorl.h solorl_terminate, termination.py)
  set_reset_randomization(**ranges), reset_randomization_count   (randomised initial states -- joint angles and velocities, base
      velocity, heading, roll and pitch drawn per env and episode on the device, the robot placed on the ground -- behind every reset:
      include/solorl.h solorl_randomize_reset / solorl_restart_history, reset_random.py)
  SoloVecEnv(..., critic_obs=True | dict), critic_obs_dim, critic_observation_space, last_critic_obs   (privileged critic rows: the clean
      observation row and twenty words of the simulator's truth -- contact forces, foot heights and speeds, the command, the episode's
      progress, collisions, the drawn latency and gain error, the last kick -- written behind every step and reset for the value
      function of an asymmetric actor-critic: include/solorl.h solorl_critic_obs, critic_obs.py)

torch is plumbing only: it owns the device buffers and the stream; all arithmetic happens in
``libsolorl_hip.so`` on the caller's current HIP stream (no host synchronisation in step()).
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from .config import SoloConfig, EnvState, InfoSoA, config_from_dict, EPSTAT_FIELDS, EPSTAT_NAMES
from .normalize import RunningMeanStd, VecNormalizer
from .rows import mask_arg, tensor_arg
from .state import StateBatch, field_bits, SF_POSE, SF_VEL, SF_JOINT_POS, SF_JOINT_VEL, SF_CONTACT

_RR_FIELDS = SF_POSE | SF_VEL | SF_JOINT_POS | SF_JOINT_VEL | SF_CONTACT      # what solorl_randomize_reset may change of a row

# The optional stages of a control step, in the order their refusals are tried: (name of the stage's ``_no_<name>`` guard, is it set on
# this env, the message's phrase, what K steps in one launch (step_n*, rollout_inplace) cannot take between the steps -- None: the stage
# does not bar them -- with the call that switches it off, what the policy inside the step kernel (step_act_inplace, rollout_inplace)
# would do wrong with it -- None: it does not bar the policy tail).  The guards, step_act_supported() and rollout_supported() read this
# table and nothing else; _before_step / _after_step hold the order the stages run in.
_STAGES = (
    ("norm_obs", lambda e: e._norm_obs, "on an env with norm_obs", None, None, "read raw observations"),
    ("kicks", lambda e: e.last_kick is not None, "with a perturbation set", "kicks", "set_perturbation(None)", None),
    ("shaping", lambda e: e._shape_params is not None, "with reward shaping set", "the shaped terms", "set_reward_shaping(None)", None),
    ("channel", lambda e: e._noise_scale is not None, "with observation noise set", "the noise launch", "set_obs_noise(None)",
     "read clean observations"),
    ("channel", lambda e: e._act is not None, "with actuation set", "the actuation launch", "set_actuation(None)", None),
    ("commands", lambda e: e._cmd is not None, "with velocity commands", "the command launch", None,
     "read the engine's rows without the command words"),
    ("termination", lambda e: e._term is not None, "with a termination set", "the termination launch", "set_termination(None)",
     "act on the observation of an env that is about to be reset"),
    ("reset_randomization", lambda e: e._rr is not None, "with a reset randomization set", "its launches behind a reset",
     "set_reset_randomization(None)", "act on the observation of the un-randomised reset"),
    ("critic_obs", lambda e: getattr(e, "_critic", None) is not None, "with critic_obs", "the critic rows' launches", None,
     "compute the value from the actor's row"),
)


class Box:
    """Stand-in for gym.spaces.Box: the policy dispatches on the class NAME
    (agents/ppo/policy.py:22-31) and reads .shape / .high / .low."""

    def __init__(self, low, high):
        self.low = np.asarray(low, dtype=np.float32)
        self.high = np.asarray(high, dtype=np.float32)
        self.shape = self.low.shape
        self.dtype = np.float32

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return np.random.uniform(lo, hi).astype(np.float32)

    def __repr__(self):
        return "Box%s" % (self.shape,)


_INFO_KEYS = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
              "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")
_DR_NAMES = {"dr_stand": "dr/stand_rew", "dr_joint_pose": "dr/joint_pose_rew", "dr_torque": "dr/torque_rew",
             "dr_balance": "dr/roll_pitch_balance_rew", "dr_progress": "dr/progress_rew"}


class LazyInfos:
    """Sequence of per-env info dicts (reference: tuple of N dicts, envs.py:94-95) backed by SoA
    device tensors; dicts are only materialised for the envs a caller actually indexes."""

    def __init__(self, tensors, done):
        self._t = tensors
        self._done = done
        self._host = None

    def _fetch(self):
        if self._host is None:
            self._host = {k: v.cpu().numpy() for k, v in self._t.items()}
        return self._host

    def __len__(self):
        return self._done.shape[0]

    def __getitem__(self, i):
        h = self._fetch()
        d = {"episode_length": int(h["episode_length"][i]), "episode_reward": float(h["episode_reward"][i]),
             "goals_reached": float(h["goals_reached"][i]),
             # keys PPO reads at done but SoloBaseEnv never sets (SURVEY 8b [BUG]) -> 0.0
             "max_velocity": 0.0, "min_force": 0.0, "max_force": 0.0, "nan_reset": bool(h["nan_reset"][i])}
        for k, name in _DR_NAMES.items():
            d[name] = float(h[k][i])
        if h["done"][i]:
            d["timeout"] = bool(h["timeout"][i])
            d["success"] = bool(h["success"][i])
        return d

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def tensors(self):
        """SoA device view: dict of [N] tensors (fast path for on-device episode statistics)."""
        return self._t


class SoloVecEnv:
    """Batched SoloBaseEnv on one MI355X.  ``config`` is a reference-style dict (configs/*.yaml)
    or a ``SoloConfig``."""

    def __init__(self, config, num_envs, device=None, seed=1, env_id_offset=0, applied_torque=False, norm_obs=False, norm_ret=False,
                 clipob=10.0, cliprew=10.0, gamma=0.99, epsilon=1e-8, commands=None, critic_obs=None, **overrides):
        self.cfg = config.copy() if isinstance(config, SoloConfig) else config_from_dict(config, **overrides)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        device = torch.device(device) if device is not None else None
        if device is not None and device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device is None or device.type != "cuda":
            raise _native.SoloRLError("SoloVecEnv needs a HIP device (got %r); the engine has no CPU fallback" % (device,))
        self.device = device
        self.L = _native.lib()
        self.nenvs = int(num_envs)
        h = C.c_void_p()
        _native.check(self.L.solorl_create(C.byref(self.cfg), self.nenvs, device.index or 0, int(seed),
                                           int(env_id_offset), C.byref(h)))
        self._h = h
        o, a, n = C.c_int(), C.c_int(), C.c_int()
        _native.check(self.L.solorl_dims(self._h, C.byref(o), C.byref(a), C.byref(n)))
        # velocity commands (``commands``: a dict of ranges, command.KEYS): the observation is the engine's row plus three command words.
        # The width is fixed here -- the normaliser below is sized by it and a policy is built from observation_space -- the ranges are
        # not (set_command_ranges).  None: nothing is allocated or launched
        self.engine_obs_dim, self.act_dim = o.value, a.value
        self._cmd = self._cmd_mem = self._cmd_all = None
        if commands is not None:
            from .command import CommandMem, make_params, ranges_from_dict
            self._cmd = make_params(seed, env_id_offset, self.engine_obs_dim, **ranges_from_dict(commands))
            self._cmd_mem = CommandMem(self.nenvs, device)
            self._cmd_all = torch.ones((self.nenvs,), dtype=torch.uint8, device=device)      # restart flags of reset()
        self.obs_dim = self.engine_obs_dim + (0 if self._cmd is None else 3)
        self.observation_space = Box(-np.inf * np.ones(self.obs_dim), np.inf * np.ones(self.obs_dim))  # baseEnv.py:27-28
        self.action_space = Box(-np.ones(self.act_dim), np.ones(self.act_dim))                          # baseEnv.py:23-25
        N = self.nenvs
        kw = dict(device=device)
        self._obs = torch.empty((N, self.obs_dim), dtype=torch.float32, **kw)
        # the rows the engine itself writes: with commands a narrow [N, D] buffer of their own, which solorl_commands widens into _obs
        self._obs_engine = self._obs if self._cmd is None else torch.empty((N, self.engine_obs_dim), dtype=torch.float32, **kw)
        self._rew = torch.empty((N,), dtype=torch.float32, **kw)
        self._done = torch.empty((N,), dtype=torch.uint8, **kw)
        self._info = {k: torch.zeros((N,), dtype=(torch.uint8 if k in ("timeout", "success", "nan_reset") else
                                                   torch.int32 if k == "episode_length" else torch.float32), **kw)
                      for k in _INFO_KEYS}
        # finished-episode accumulators [fields][N], updated by the step kernel itself (include/solorl.h ep_stats)
        self._ep_stats = torch.zeros((EPSTAT_FIELDS, N), dtype=torch.float32, **kw)
        # the torques the step applied (include/solorl.h applied_torque): allocated on request only (record_applied_torque())
        # (constructor flag `applied_torque`, or record_applied_torque() before the first step: the pointer is a kernel argument, and a HIP
        # graph captured earlier would keep replaying the NULL it was captured with)
        self._tau = torch.zeros((N, self.act_dim), dtype=torch.float32, **kw) if applied_torque else None
        self._steps_issued = 0
        self._push_states = None    # engine-owned StateBatch of push(), allocated at its first call
        self._kin_states = None     # engine-owned StateBatch of get_kinematics(), allocated at its first call
        self._dyn_states = None     # engine-owned StateBatch of get_dynamics(), allocated at its first call
        self._kbuf = {}             # engine-owned [K, ...] rows of step_n_inplace / rollout_inplace, per K
        self.last_kick = None       # [N, 6] float64: the kick of the last perturb(), allocated by set_perturbation(); None = no perturbation set
        # reward shaping (set_reward_shaping): nothing is allocated or launched unless it is set
        self._shape_params = None   # ShapeParams; None = shaping off
        self._shape_mem = None      # ShapeMem: the per-env memory of the shaped terms
        self._shape_states = None   # engine-owned StateBatch the state after each step is read into
        self._shape_ep = None       # [17, N] float64: finished episodes and their weighted term sums, per env
        self.last_shaping_terms = None   # [N, 16] float64: the raw term values of the last step (zeros for an env that finished)
        # observation noise and actuation (set_obs_noise, set_actuation): nothing is allocated or launched unless they are set
        self._seed, self._id0 = int(seed), int(env_id_offset)     # the key and the global env ids of their Philox streams
        self._noise_scale = None    # [O] float32: the noise half-width per observation component; None = noise off
        self._noise_count = None    # [N] int32 (uint32 words): the noise calls each env has received
        self._act = None            # Actuation; None = actuation off
        self._act_mem = None        # ActuatorMem: the per-env delay line, gains and latency
        self._act_restart = None    # [N] uint8: the envs whose next action is the first of an episode
        self.last_applied_actions = None   # [N, A] float32: what the last step launch received for the caller's raw actions
        # early termination (set_termination): nothing is allocated or launched unless it is set
        self._term = None           # Termination; None = early termination off
        self._term_states = None    # engine-owned StateBatch the state after each step is read into (shared with the shaped terms)
        self._term_stats = None     # [5, N] float32: early terminations and the rules that fired in them, per env
        self._term_eps = None       # [2] float64: finished episodes already flushed out of ep_stats, and the ep_stats count they start from
        self.last_termination = None   # [N] uint8: the rule bits that ended each env's episode in the last step, 0 where none
        # randomised initial states (set_reset_randomization): nothing is allocated or launched unless it is set
        self._rr = None             # ResetRandomization; None = the engine's own snapshots
        self._rr_states = None      # engine-owned StateBatch the freshly reset envs are read into and written back from
        self._rr_all = None         # [N] uint8 of ones: the mask of reset()
        self.reset_randomization_count = None   # [N] int32 (uint32 words): the episodes each env has drawn an initial state for
        self._info_c = InfoSoA(ep_stats=self._ep_stats.data_ptr(), applied_torque=None if self._tau is None else self._tau.data_ptr(),
                               **{k: self._info[k].data_ptr() for k in _INFO_KEYS})
        self._info_alt = {}         # timeout_out pointer -> _info_c with its timeout flags going there (_info_block)
        # VecNormalize (agents/running_mean_std.py:73-127; the reference's launcher passes ob=False, ret=False: agents/ppo/envs.py:26):
        # nothing is allocated or launched unless a switch is on
        self._norm = VecNormalizer(N, self.obs_dim, device, norm_obs, norm_ret, clipob, cliprew, gamma, epsilon) if (norm_obs or norm_ret) else None
        self._norm_obs, self._norm_ret = bool(norm_obs), bool(norm_ret)
        # privileged critic rows (``critic_obs``: True, or a dict of scale overrides, critic_obs.GROUPS): the engine's clean row plus
        # twenty words.  The width is fixed here, as with commands -- a policy is built from critic_observation_space.  None or False:
        # nothing is allocated or launched
        self._critic = self._critic_states = self._critic_clean = self.last_critic_obs = None
        self.critic_obs_dim = self.critic_observation_space = None
        if critic_obs is not None and critic_obs is not False:
            from .critic_obs import CRITIC_PRIV, make_params, scales_from_dict
            if norm_obs:
                raise _native.SoloRLError("critic_obs on an env with norm_obs: the critic rows would need running statistics of their own "
                                          "(normalise the rows in the policy, or leave norm_obs off)")
            self._critic = make_params(self.cfg, self.engine_obs_dim, **(scales_from_dict(critic_obs) if isinstance(critic_obs, dict) else {}))
            self.critic_obs_dim = self.engine_obs_dim + CRITIC_PRIV
            self.critic_observation_space = Box(-np.inf * np.ones(self.critic_obs_dim), np.inf * np.ones(self.critic_obs_dim))
            self._critic_states = StateBatch(N, device)    # engine-owned: the state the new observation describes
            # the engine's rows before the noise, while noise is set: the engine writes these and solorl_obs_noise the caller's, out of place
            self._critic_clean = torch.zeros((N, self.engine_obs_dim), dtype=torch.float32, **kw)
            self.last_critic_obs = torch.zeros((N, self.critic_obs_dim), dtype=torch.float32, **kw)
        self.training = True        # running_mean_std.py:94
        self.closed = False

    # reference call path: PyTorchEnvWrapper.envs (VecNormalize) .venv ...
    @property
    def envs(self):
        return self

    @property
    def venv(self):
        return self

    def __len__(self):
        return self.nenvs

    # ---- VecNormalize: the statistics live on the device; ob_rms / ret_rms are host copies (one device -> host copy per read), and
    # assigning one (`env.envs.ob_rms = ckpt['ob_rms']`, testing/test_ppo.py:89-90) uploads it
    @property
    def ob_rms(self):
        return RunningMeanStd(shape=(self.obs_dim,)).from_device(self._norm.ob_stats) if self._norm_obs else None

    @ob_rms.setter
    def ob_rms(self, rms):
        if rms is None and not self._norm_obs:
            return
        if rms is None or not self._norm_obs:
            raise _native.SoloRLError("ob_rms can only be assigned statistics on an env made with norm_obs=True (and never None on one)")
        rms.to_device(self.device, out=self._norm.ob_stats)

    @property
    def ret_rms(self):
        return RunningMeanStd(shape=()).from_device(self._norm.ret_stats) if self._norm_ret else None

    @ret_rms.setter
    def ret_rms(self, rms):
        if rms is None and not self._norm_ret:
            return
        if rms is None or not self._norm_ret:
            raise _native.SoloRLError("ret_rms can only be assigned statistics on an env made with norm_ret=True (and never None on one)")
        rms.to_device(self.device, out=self._norm.ret_stats)

    def eval(self):
        """running_mean_std.py:123-124: the statistics stop updating (the scaling goes on)"""
        self.training = False

    def train(self):
        self.training = True

    def normalize_obs(self, obs, update=False):
        """What the policy sees for raw observations [N, O] (get_observation() stays raw, as the reference's wrapper leaves it): a
        normalised copy, the statistics untouched unless ``update``.  Identity without norm_obs."""
        if not self._norm_obs:
            return obs
        x = obs.detach().to(device=self.device, dtype=torch.float32).contiguous()
        return self._norm.obs(x, 1, update, out=torch.empty_like(x))

    def _normalize(self, o, r, d, rows, obs=True):
        """The wrapper's half of a step (running_mean_std.py:96-107) on the `rows` rows the engine has just written, in place
        (``obs=False``: the rewards only)."""
        if self._norm_obs and obs:
            self._norm.obs(o, rows, self.training)
        if self._norm_ret:
            self._norm.rewards(r, d, rows, self.training)

    def _refuse(self, name, k_step=False, tail=False, guard=None):
        """Raises for the first stage of _STAGES (of those with guard name ``guard``, if given) that is set on this env and bars ``name``:
        a launch of K steps (``k_step``) or one with the policy inside the step kernel (``tail``)"""
        for g, is_set, phrase, between, off, policy in _STAGES:
            if guard not in (None, g) or not is_set(self):
                continue
            if tail and policy is not None:
                raise _native.SoloRLError("%s %s: the policy inside the step kernel would %s (step_act_supported() / rollout_supported() "
                                          "are False)" % (name, phrase, policy))
            if k_step and between is not None:
                raise _native.SoloRLError("%s %s: K steps in one launch cannot take %s between the steps (rollout_supported() is False; "
                                          "step one at a time%s)" % (name, phrase, between, "" if off is None else ", or " + off))

    def _no_policy_tail(self, name):
        self._refuse(name, tail=True)

    def _stream(self):
        return _native.stream(self.device)

    # ---- device-side kicks (include/solorl.h solorl_set_perturbation / solorl_perturb / solorl_get_perturbation)
    def set_perturbation(self, interval, max_lin_vel=0.0, max_ang_vel=0.0):
        """Random base kicks during stepping: every env is kicked every ``interval`` control steps (an int, or a (lo, hi) pair: uniform
        in lo..hi, drawn per env and kick), the kick adding U(-m, m) per component to the base's world-frame linear / angular velocity
        (``max_lin_vel`` / ``max_ang_vel``: a scalar or a 3-sequence; 0 = that component is never touched).  Drawn on the device from a
        Philox stream per env (the draw table is in include/solorl.h); calling it again restarts the schedule, ``interval=None``
        switches it off.  Synchronises the host; call it before capturing a HIP graph of steps.

        While a perturbation is set, step(), step_inplace() and step_act_inplace() issue perturb() right before their step launch, so a
        control step is  observation -> policy -> kick -> physics:  a kick is a disturbance of the transition, the policy sees it in the
        next observation (also in step_act_inplace, whose tail computes the next action from the observation AFTER the kicked step).
        step_n*, rollout_inplace run K steps in one launch and cannot take kicks in between: they raise, and rollout_supported() is False."""
        if interval is None:
            with torch.cuda.device(self.device):
                _native.check(self.L.solorl_set_perturbation(self._h, None))
            self.last_kick = None
            return
        lo, hi = (interval, interval) if np.isscalar(interval) else interval
        if int(lo) != lo or int(hi) != hi:
            raise AssertionError("interval must be an int or a pair of ints, got %r" % (interval,))

        def amp(x):
            v = np.broadcast_to(np.asarray(x, dtype=np.float64), (3,)) if np.ndim(x) == 0 else np.asarray(x, dtype=np.float64)
            if v.shape != (3,):
                raise AssertionError("an amplitude is a scalar or a 3-sequence, got %r" % (x,))
            return (C.c_double * 3)(*v.tolist())
        p = _native.Perturbation(int(lo), int(hi), amp(max_lin_vel), amp(max_ang_vel))
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_set_perturbation(self._h, C.byref(p)))
        if self.last_kick is None:
            self.last_kick = torch.zeros((self.nenvs, 6), dtype=torch.float64, device=self.device)
        else:
            self.last_kick.zero_()

    def perturb(self):
        """One solorl_perturb launch on the current stream: every env's countdown goes down by one, the envs that reach 0 are kicked.
        -> last_kick [N, 6] (lin x y z, ang x y z; zeros for the envs not kicked by this call).  No host synchronisation: capturable."""
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_perturb(self._h, None if self.last_kick is None else C.c_void_p(self.last_kick.data_ptr()), self._stream()))
        return self.last_kick

    def perturbation_state(self):
        """(countdown int32 [N], kicks drawn so far [N] as int64 -- the engine's uint32 widened) of the kick schedule, by env id"""
        cd = torch.empty((self.nenvs,), dtype=torch.int32, device=self.device)
        kc = torch.empty((self.nenvs,), dtype=torch.int32, device=self.device)     # (uint32 words: torch has no arithmetic on that type)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_get_perturbation(self._h, C.c_void_p(cd.data_ptr()), C.c_void_p(kc.data_ptr()), self._stream()))
        return cd, kc.to(torch.int64) & 0xFFFFFFFF

    def _kick(self):
        """the kick of a control step, in front of its step launch"""
        if self.last_kick is not None:
            self.perturb()

    # ---- shaped reward terms (include/solorl.h solorl_shape_reward; shaping.py)
    def set_reward_shaping(self, weights, **params):
        """Adds the shaped terms named in ``weights`` (dict term name -> weight, shaping.TERMS; the table is in include/solorl.h) to every
        step's reward; ``params``: base_height_target, foot_clearance_target, foot_force_max, air_time_target, cmd_lin_vel, cmd_yaw_rate,
        tracking_sigma (shaping.PARAM_DEFAULTS).  ``weights=None`` switches it off.  Allocates the per-env memory (ShapeMem), an
        engine-owned StateBatch, ``last_shaping_terms`` [N, 16] and the finished-episode sums [17, N] at the first call and clears them
        at every call; call it before capturing a HIP graph of steps (the weights are launch arguments).

        While set, step(), step_inplace() and step_act_inplace() issue get_states and ONE solorl_shape_reward launch right behind their
        step launch, on the same stream and without host synchronisation, before the return normalisation -- which therefore sees the
        shaped reward.  An env that finished in the step keeps the engine's terminal reward.  The torques and power terms read the state
        row's ``tau``, which solorl_get_states leaves 0: they are 0 unless the env records the applied torques (``applied_torque=True``),
        which are then copied into the rows in front of the launch.  step_n*, rollout_inplace run K steps in one
        launch and cannot take the launch in between: they raise, and rollout_supported() is False."""
        from .shaping import EP_FIELDS, SHAPE_TERMS, ShapeMem, make_params
        if weights is None:
            self._shape_params = self._shape_mem = self._shape_states = self._shape_ep = self.last_shaping_terms = None
            return
        p = make_params(weights, **params)
        if self._shape_mem is None:
            self._shape_mem = ShapeMem(self.nenvs, self.device)
            self._shape_states = StateBatch(self.nenvs, self.device)
            self._shape_ep = torch.zeros((EP_FIELDS, self.nenvs), dtype=torch.float64, device=self.device)
            self.last_shaping_terms = torch.zeros((self.nenvs, SHAPE_TERMS), dtype=torch.float64, device=self.device)
        else:
            for t in (self._shape_mem.data, self._shape_ep, self.last_shaping_terms):
                t.zero_()
        self._shape_params = p

    def _shape(self, actions, rew, done, rows=None):
        """the shaped terms of a control step, behind its step launch: the state after the step (``rows``: the rows _terminate has
        already read, taken before its reset), then one launch -> the rows it read, or ``rows``"""
        if self._shape_params is not None:
            from .shaping import shape_reward
            if rows is None:
                rows = self.get_states(out=self._shape_states)
            if self._tau is not None:                   # solorl_get_states leaves `tau` 0: the torques and power terms read the recorded torques
                rows.tau[:, :self.act_dim].copy_(self._tau)
            shape_reward(self.cfg, self._shape_params, rows, actions, done, self._shape_mem, rew,
                         terms_out=self.last_shaping_terms, ep_out=self._shape_ep, commands=self._cmd_mem)
        return rows

    def shaping_stats(self, reset=True):
        """Means over the episodes finished since the last call of each term's weighted sum over the episode, ``sr/<name>``, and their
        count ``episodes`` -- reduced on the device from the per-env sums solorl_shape_reward keeps; one small device->host copy.
        ``reset`` zeroes the sums."""
        from .shaping import TERMS
        if self._shape_ep is None:
            raise _native.SoloRLError("shaping_stats() without reward shaping set")
        tot = self._shape_ep.sum(dim=1)
        if reset:
            self._shape_ep.zero_()
        tot = tot.tolist()
        n = tot[0]
        out = {"episodes": int(n)}
        for k, name in enumerate(TERMS):
            out["sr/" + name] = (tot[1 + k] / n) if n > 0 else float("nan")
        return out

    # ---- early termination (include/solorl.h solorl_terminate; termination.py)
    def set_termination(self, rules=None, **more):
        """Ends an episode early when the state after a step breaks a rule: ``base_height`` [m], ``max_tilt_deg``, ``contacts`` (group
        names ``base``, ``knees``, ``shoulders`` or primitive indices) with ``contact_force_min`` [N], ``joint_limits`` ([lo, hi], or one
        pair per joint), and ``min_steps``, ``terminal_reward`` (default -10) -- termination.make_termination; a rule is enabled by
        naming its key, as keywords or as one dict.  ``set_termination(None)`` switches it off.  Allocates ``last_termination`` (uint8 [N]:
        the rule bits that ended each env's episode in the last step), the statistics block and an engine-owned StateBatch at the first
        call and clears them at every call; call it before capturing a HIP graph of steps (the rules are launch arguments).

        While set, step() and step_inplace() issue, right behind their step launch and on the same stream: get_states (one launch,
        shared with the shaped reward terms when those are set), ONE solorl_terminate launch on the step's done flags, reward and info
        arrays, and solorl_reset_masked(last_termination) into the observation rows the engine has just written.  Everything behind it
        sees the merged done flags: the shaped terms (on the rows taken before the reset: they leave the terminal reward alone and flush
        their episode sums), actuation and commands (the env restarts its episode), return normalisation (a new return starts).  The
        policy inside the step kernel would act on the observation of an env that is about to be reset, so step_act_supported() and
        rollout_supported() are False, step_act_inplace() raises, and so do step_n*, rollout_inplace (K steps in one launch)."""
        from .termination import STAT_FIELDS, make_termination
        if rules is None and not more:
            self._term = self._term_states = self._term_stats = self._term_eps = self.last_termination = None
            return
        p = make_termination(self.cfg, **dict(rules or {}, **more))
        if self._term_states is None:
            self._term_states = StateBatch(self.nenvs, self.device)
            self._term_stats = torch.zeros((STAT_FIELDS, self.nenvs), dtype=torch.float32, device=self.device)
            self._term_eps = torch.zeros((2,), dtype=torch.float64, device=self.device)
            self.last_termination = torch.zeros((self.nenvs,), dtype=torch.uint8, device=self.device)
        else:
            for t in (self._term_stats, self._term_eps, self.last_termination):
                t.zero_()
        self._term_eps[1] = self._ep_stats[0].sum(dtype=torch.float64)      # episodes finished before now are not this termination's
        self._term = p

    def _terminate(self, e, rew, done, info=None):
        """the early termination of a control step, behind its step launch: the state after the step, one launch on the step's
        outputs (``info``: the block the step launch was given, default the engine-owned one -- a rule-ended env reads timeout == 0
        wherever the step wrote its flags), and the reset of the envs it ended into the engine's observation rows ``e`` -> the rows
        (pre-reset) or None"""
        if self._term is None:
            return None
        from .termination import terminate
        rows = self.get_states(out=self._term_states)
        terminate(self.cfg, self._term, rows, done, rew, self.last_termination, info=self._info_c if info is None else info,
                  term_stats=self._term_stats)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_reset_masked(self._h, C.c_void_p(self.last_termination.data_ptr()), C.c_void_p(e.data_ptr()), self._stream()))
        return rows

    def termination_stats(self, reset=True):
        """``term/episodes``: the episodes finished since the last call, by any cause; ``term/early``: the share of them that a rule
        ended, and ``term/<rule>`` (height, tilt, contact, joint; the enabled ones): the share each rule ended -- an episode that
        several rules ended at once counts for each.  Reduced on the device from the per-env counts solorl_terminate keeps and the
        engine's finished-episode count; one small device->host copy.  ``reset`` starts the next window."""
        from .termination import RULES
        if self._term is None:
            raise _native.SoloRLError("termination_stats() without a termination set")
        cur = self._ep_stats[0].sum(dtype=torch.float64)
        tot = torch.cat([self._term_stats.sum(dim=1, dtype=torch.float64), (self._term_eps[0] + cur - self._term_eps[1]).reshape(1)])
        if reset:
            self._term_stats.zero_()
            self._term_eps[0] = 0.0
            self._term_eps[1] = cur
        tot = tot.tolist()
        n = tot[-1]
        out = {"term/episodes": int(n), "term/early": (tot[0] / n) if n > 0 else float("nan")}
        for k, name in enumerate(RULES):
            if (self._term.rules >> k) & 1:
                out["term/" + name] = (tot[1 + k] / n) if n > 0 else float("nan")
        return out

    # ---- randomised initial states (include/solorl.h solorl_randomize_reset / solorl_restart_history; reset_random.py)
    def set_reset_randomization(self, ranges=None, **more):
        """Every episode starts from a randomised state: half-widths ``joint_pos`` [rad] and ``joint_vel`` [rad/s] (a scalar or one value per
        joint), ``lin_vel`` [m/s] and ``ang_vel`` [rad/s] (a scalar or x, y, z; world frame), ``yaw``, ``roll``, ``pitch`` [rad], and
        ``place_on_ground`` (default True) with ``clearance`` [m] -- reset_random.make_reset_randomization; as keywords or as one dict.
        ``set_reset_randomization(None)`` switches it off.  Allocates an engine-owned StateBatch and ``reset_randomization_count``
        (int32 [N]: the episodes each env has drawn for) at the first call and zeroes the count at every call; call it before capturing
        a HIP graph of steps (the ranges are launch arguments).

        While set, four launches on the same stream follow every reset of an env -- get_states(mask), ONE solorl_randomize_reset,
        solorl_set_states(mask, pose | vel | joint_pos | joint_vel | contact) and solorl_restart_history(mask) into the observation rows
        the engine has just written -- with mask = the merged done flags in step() and step_inplace(), every env in reset(), the selected
        envs in reset_masked().  In a step they stand behind the shaped terms and in front of the noise: the shaped terms and the
        termination see what they see without it; noise, commands and normalisation see the randomised first observation, whose delta
        words are exactly 0 and whose four feet words are 0 (the contact cache is dropped with the pose).  The policy inside the step
        kernel would act on the observation of the un-randomised reset, so step_act_supported() and rollout_supported() are False,
        step_act_inplace() raises, and so do step_n*, rollout_inplace (K steps in one launch)."""
        from .reset_random import make_reset_randomization
        if ranges is None and not more:
            self._rr = self._rr_states = self._rr_all = self.reset_randomization_count = None
            return
        p = make_reset_randomization(self.cfg, self._seed, self._id0, **dict(ranges or {}, **more))
        if self._rr_states is None:
            self._rr_states = StateBatch(self.nenvs, self.device)
            self._rr_all = torch.ones((self.nenvs,), dtype=torch.uint8, device=self.device)
            self.reset_randomization_count = torch.zeros((self.nenvs,), dtype=torch.int32, device=self.device)
        else:
            self.reset_randomization_count.zero_()
        self._rr = p

    def _randomize(self, e, mask):
        """the randomised initial state of the envs ``mask`` selects (uint8 [N]: they have just been reset), and their rows of the
        engine's observation rows ``e``"""
        if self._rr is None:
            return
        from .reset_random import randomize_reset
        rows = self.get_states(mask, out=self._rr_states)
        randomize_reset(self.cfg, self._rr, rows, self.reset_randomization_count, mask=mask)
        self.set_states(rows, mask, _RR_FIELDS)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_restart_history(self._h, C.c_void_p(mask.data_ptr()), C.c_void_p(e.data_ptr()), self._stream()))

    # ---- observation noise and actuation (include/solorl.h solorl_obs_noise / solorl_actuate; channel.py)
    def set_obs_noise(self, scales):
        """Uniform sensor noise on every observation the engine hands out: ``scales`` is a dict of half-widths in physical units per
        group (channel.noise_scales: height, orientation, lin_vel, ang_vel, joint_pos, joint_vel, position; or a noise file's dict with
        ``groups`` and ``history``, configs/noise_solo.yaml) or an ``[obs_dim]`` vector of half-widths in the observation's own units.
        ``None`` switches it off.  Calling it again restarts every env's noise stream.  Allocates its two arrays here: call it before
        capturing a HIP graph of steps.

        While set, reset(), step(), step_inplace() and reset_masked() (the selected rows) issue ONE solorl_obs_noise launch on the
        observation rows the engine has just written, in place, before the observation normalisation -- rollout-storage rows hold what
        the policy saw; get_observation() stays clean.  The policy inside the step kernel would read clean observations, so
        step_act_supported() and rollout_supported() are False, step_act_inplace() raises, and so do step_n*, rollout_inplace (K steps in
        one launch)."""
        from .channel import noise_scales, scales_from_dict
        if scales is None:
            self._noise_scale = self._noise_count = None
            return
        if isinstance(scales, dict):
            v = scales_from_dict(self.cfg, scales) if "groups" in scales else noise_scales(self.cfg, scales)
        else:
            v = torch.as_tensor(scales, dtype=torch.float32).detach().reshape(-1)
        if tuple(v.shape) != (self.engine_obs_dim,) or not bool(torch.isfinite(v).all()) or bool((v < 0).any()):
            raise AssertionError("observation noise scales must be %d finite values >= 0" % self.engine_obs_dim)
        self._noise_scale = v.to(self.device).contiguous()
        if self._noise_count is None:
            self._noise_count = torch.zeros((self.nenvs,), dtype=torch.int32, device=self.device)
        else:
            self._noise_count.zero_()

    def _noise(self, o, mask=None, out=None):
        """the sensor noise of the observation rows the engine has just written, in place (``out``: into these rows, ``o`` staying clean)"""
        if self._noise_scale is not None:
            from .channel import obs_noise
            obs_noise(self._seed, self._id0, self._noise_scale, self._noise_count, o, out=None if out is o else out, mask=mask)

    def set_actuation(self, delay=None, gain_range=0.0):
        """Actuation latency and motor gain error between the caller's actions and the engine: every env applies the action it received
        ``delay`` control steps ago (an int, or a (lo, hi) pair within 0..4: uniform, drawn per env and episode; until that many actions
        have arrived in an episode its first action is held), each joint's action scaled by a gain 1 + U(-gain_range, gain_range) drawn
        per env, episode and joint.  ``delay=None`` with ``gain_range=0`` switches it off.  Calling it again starts every env over (episode 0's
        draws, empty delay lines).  Allocates its buffers here: call it before capturing a HIP graph of steps.

        While set, step(), step_inplace() and step_act_inplace() issue ONE solorl_actuate launch in front of the kick and the step
        launch: it reads the caller's actions, which are never written, and writes ``last_applied_actions`` [N, A], which the step launch
        receives.  Rollout storage and the shaped reward terms keep the raw actions.  An env restarts its episode draws after a step that
        finished it, after reset() and after reset_masked() selected it.  step_act_inplace() stays supported (the tail's action is raw and
        is delayed at the next call); step_n*, rollout_inplace raise, and rollout_supported() is False."""
        from .channel import ActuatorMem, make_actuation
        if delay is None and not gain_range:
            self._act = self._act_mem = self._act_restart = self.last_applied_actions = None
            return
        p = make_actuation(self._seed, self._id0, self.act_dim, 0 if delay is None else delay, gain_range)
        if not (0 <= p.delay_min <= p.delay_max <= _native.DELAY_MAX) or not (0.0 <= p.gain_range < 1.0):
            raise AssertionError("delay must lie within 0..%d and gain_range in [0, 1), got %r, %r" % (_native.DELAY_MAX, delay, gain_range))
        if self._act_mem is None:
            self._act_mem = ActuatorMem(self.nenvs, self.device)
            self._act_restart = torch.ones((self.nenvs,), dtype=torch.uint8, device=self.device)
            self.last_applied_actions = torch.zeros((self.nenvs, self.act_dim), dtype=torch.float32, device=self.device)
        else:
            self._act_mem.data.zero_()
            self._act_restart.fill_(1)
            self.last_applied_actions.zero_()
        self._act = p

    def _actuate(self, actions):
        """the actions a step launch receives for the caller's raw ``actions`` [N, A]: themselves, or the delayed and scaled ones"""
        if self._act is None:
            return actions
        from .channel import actuate
        return actuate(self._act, self._act_mem, actions, out=self.last_applied_actions, restart=self._act_restart)

    def _restarts(self, done):
        """behind a step launch: the envs it finished start an episode with their next action"""
        if self._act is not None:
            self._act_restart.copy_(done)

    # ---- velocity commands (include/solorl.h solorl_commands; command.py)
    @property
    def last_commands(self):
        """[N, 3] float64 view of the command rows: the command (vx, vy, yaw rate) every env holds now; None without commands"""
        return None if self._cmd is None else self._cmd_mem.cmd

    def set_command_ranges(self, **ranges):
        """Changes what later draws use: ``lin_vel_x``, ``lin_vel_y``, ``yaw_rate`` ([lo, hi] pairs or fixed numbers), ``interval``,
        ``zero_prob``, ``min_lin_norm``, ``obs_scale`` (command.KEYS); what is not named stays.  The parameters go to every launch by
        value, so a command curriculum is a host loop around this call -- but a HIP graph captured earlier keeps the values it was
        captured with.  Every env's countdown is set to 1 (one small fill on the device), so every env draws from the new ranges at its
        next step: ``lo == hi`` with ``interval=1`` is joystick control, every env holding exactly that command after the next step.  The
        width of the observation does not change."""
        from .command import make_params, ranges_of
        if self._cmd is None:
            raise _native.SoloRLError("set_command_ranges() on an env made without commands (the observation width is fixed at construction: "
                                      "SoloVecEnv(..., commands=dict))")
        self._cmd = make_params(self._seed, self._id0, self.engine_obs_dim, **dict(ranges_of(self._cmd), **ranges))
        self._cmd_mem.countdown.fill_(1)

    def _commands(self, o, restart, mask=None):
        """the command step of the engine's rows: the wide rows ``o`` [N, D + 3] = _obs_engine and each env's command words, the envs
        of ``restart`` (and those whose countdown runs out) drawing a new command first"""
        if self._cmd is not None:
            from .command import commands
            commands(self._cmd, self._cmd_mem, self._obs_engine, out=o, restart=restart, mask=mask)

    def _command_words(self):
        """[N, 3] float32: the observation words of the commands held now (torch ops: not on the hot path)"""
        scale = torch.tensor(list(self._cmd.obs_scale), dtype=torch.float64, device=self.device)
        return (self._cmd_mem.cmd * scale).to(torch.float32)

    # ---- privileged critic rows (include/solorl.h solorl_critic_obs; critic_obs.py)
    def _clean_rows(self, e):
        """the rows the engine writes for the caller's engine rows ``e``: ``e`` itself, or -- with critic rows and noise both set -- the
        clean buffer, from which solorl_obs_noise writes ``e`` out of place"""
        return self._critic_clean if self._critic is not None and self._noise_scale is not None else e

    def _critic_rows(self, clean, out=None, rows=None):
        """the critic rows of the observation just written, behind every other stage: the state that observation describes (``rows``:
        rows already read in this step that are still current; else a get_states of its own), then one launch on the engine's clean
        rows ``clean``, the command, actuator and kick rows the env holds now -> ``out`` (default: last_critic_obs)"""
        if self._critic is None:
            return None
        from .critic_obs import critic_obs
        if rows is None:
            rows = self.get_states(out=self._critic_states)
        return critic_obs(self.cfg, self._critic, rows, clean, out=self.last_critic_obs if out is None else out, commands=self._cmd_mem,
                          actuators=self._act_mem, kick=self.last_kick)

    def reset(self):
        c = self._clean_rows(self._obs_engine)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_reset(self._h, C.c_void_p(c.data_ptr()), self._stream()))
        if self._act is not None:                       # every env starts an episode
            self._act_restart.fill_(1)
        self._randomize(c, self._rr_all)
        self._noise(c, out=self._obs_engine)
        self._commands(self._obs, self._cmd_all)        # every env draws a command
        self._critic_rows(c)
        if self._shape_mem is not None:                 # every env starts an episode
            self._shape_mem.data.zero_()
        if self.last_termination is not None:
            self.last_termination.zero_()
        if self._norm is not None:                      # running_mean_std.py:118-121
            self._norm.ret.zero_()
            if self._norm_obs:
                self._norm.obs(self._obs, 1, self.training)
        return self._obs.clone()

    def step(self, actions):
        if actions.shape != (self.nenvs, self.act_dim):
            raise AssertionError("actions must be [%d, %d]" % (self.nenvs, self.act_dim))   # solo.py:226
        a = actions.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.step_inplace(a)                            # (on the engine-owned buffers)
        t = {k: v.clone() for k, v in self._info.items()}
        t["done"] = self._done.clone()
        return self._obs.clone(), self._rew.clone().unsqueeze(-1), t["done"].float(), LazyInfos(t, t["done"])

    def _before_step(self, actions):
        """in front of a step launch: the actuation, then the kick -> the actions the launch receives for the caller's raw ``actions``"""
        applied = self._actuate(actions)
        self._kick()
        return applied

    def _after_step(self, e, o, r, d, actions, tail=False, clean=None, critic_out=None, info=None):
        """behind a step launch that wrote the engine's observation rows ``e``, rewards ``r`` and done flags ``d``: every stage that is
        set, in the one order there is; ``o``: the caller's observation rows (``e`` without commands).  ``tail``: the subset of
        step_act_inplace -- restarts, shaped terms, return normalisation -- whose policy has already read ``o``.  ``clean``: the rows
        the launch wrote instead of ``e`` (_clean_rows: the noise then writes ``e`` from them); ``critic_out``: where the critic rows go;
        ``info``: the info block the launch was given (_info_block), which the early termination books into"""
        c = e if clean is None else clean
        rows = None if tail else self._terminate(c, r, d, info)
        self._restarts(d)
        rows = self._shape(actions, r, d, rows)         # (with commands: against the command the policy acted on, before it is redrawn)
        if not tail:
            self._randomize(c, d)
            self._noise(c, out=e)
            self._commands(o, d)
            # (rows read behind the step are the state the observation describes unless a termination or a randomised start has reset envs since)
            self._critic_rows(c, critic_out, rows if self._term is None and self._rr is None else None)
        if self._norm is not None:
            self._normalize(o, r, d, 1, obs=not tail)

    def _raw(self, name, x, *shapes, dtype=torch.float32):
        """The C ABI takes raw pointers: `x` must already be `dtype`, contiguous, of one of `shapes`, on this env's device."""
        return tensor_arg(name, x, shapes, dtype, self.device)

    def _per_env(self, name, x, lead):
        """one float per env and row (rewards, values, log-probs): [.., N] or [.., N, 1]"""
        return self._raw(name, x, lead + (self.nenvs,), lead + (self.nenvs, 1))

    def _outputs(self, lead, own, obs_out, rew_out, done_out):
        """Output tensors of a step call with leading shape `lead` = () or (K,): the caller's, or the engine-owned defaults `own` =
        (obs, rew, done) -> (o, r, d, and their checked pointers): observations lead + [N, O], rewards lead + [N] or [N, 1], done
        flags uint8 lead + [N]."""
        o, r, d = (own[i] if x is None else x for i, x in enumerate((obs_out, rew_out, done_out)))
        return (o, r, d, self._raw("obs_out", o, lead + (self.nenvs, self.obs_dim)), self._per_env("rew_out", r, lead),
                self._raw("done_out", d, lead + (self.nenvs,), dtype=torch.uint8))

    def _info_block(self, base, tensors, alt, timeout_out, lead):
        """The info block and the info tensors of a launch: the engine-owned ``base`` / ``tensors``, or -- with ``timeout_out``, a
        caller-owned uint8 lead + [N] or [N, 1] tensor such as a rollout-storage row -- a copy of the block whose ``timeout`` pointer is
        the caller's row, and the tensors with that row under "timeout".  The C ABI takes the info pointers per call, so the flags
        land in the caller's row by the step launch itself: no copy, no further launch.  The copies are kept in ``alt`` per
        destination pointer (a rollout storage has T of them)."""
        if timeout_out is None:
            return base, tensors
        p = self._raw("timeout_out", timeout_out, lead + (self.nenvs,), lead + (self.nenvs, 1), dtype=torch.uint8).value
        c = alt.get(p)
        if c is None:
            if len(alt) >= 4096:                        # (a caller that hands over a new tensor at every step)
                alt.clear()
            c = alt[p] = InfoSoA.from_buffer_copy(base)
            c.timeout = p
        return c, dict(tensors, timeout=timeout_out)

    def step_inplace(self, actions, obs_out=None, rew_out=None, done_out=None, critic_obs_out=None, timeout_out=None):
        """Zero-copy variant for rollout loops: returns views of the engine-owned output buffers (overwritten by the next
        step) -- or writes observations [N, O] / rewards [N] or [N, 1] / done flags (uint8 [N]) straight into caller-owned tensors
        such as rollout-storage rows (the C ABI takes the caller's pointers anyway).  Host-side checks only, capturable in a HIP graph.
        With velocity commands O is the wide width: the engine writes its own narrow buffer and solorl_commands the caller's rows.
        ``critic_obs_out`` (an env made with critic_obs): where the critic rows [N, critic_obs_dim] go instead of last_critic_obs.
        ``timeout_out`` (uint8 [N] or [N, 1]): where the step's timeout flags go instead of the engine-owned info["timeout"] -- the
        returned info then holds that row.  The flag is 1 where the time limit ended the episode (tested first: a fall on the very last
        step is a timeout) and 0 for every other env, one that a termination rule, the NaN guard or a reached goal ended included."""
        a = self._raw("actions", actions, (self.nenvs, self.act_dim))
        o, r, d, po, pr, pd = self._outputs((), (self._obs, self._rew, self._done), obs_out, rew_out, done_out)
        ic, info = self._info_block(self._info_c, self._info, self._info_alt, timeout_out, ())
        if critic_obs_out is not None:
            if self._critic is None:
                raise _native.SoloRLError("critic_obs_out on an env made without critic_obs (the width is fixed at construction: "
                                          "SoloVecEnv(..., critic_obs=True))")
            self._raw("critic_obs_out", critic_obs_out, (self.nenvs, self.critic_obs_dim))
        e = o if self._cmd is None else self._obs_engine
        c = self._clean_rows(e)
        self._steps_issued += 1
        applied = self._before_step(actions)
        if applied is not actions:
            a = C.c_void_p(applied.data_ptr())
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_step(self._h, a, C.c_void_p(c.data_ptr()), pr, pd, C.byref(ic), self._stream()))
        self._after_step(e, o, r, d, actions, clean=c, critic_out=critic_obs_out, info=ic)
        return o, r, d, info

    def step_act_supported(self, params):
        """The policy tail's prerequisites (solorl_step_act, solorl_rollout; include/solorl.h), decided from the handle -- what the engine
        latched at solorl_create, whatever the environment says now: fp32, team mode, no sorting, and an observation size that is a
        multiple of 4 floats and at most 88 (zero or one history level) with the reference's hidden-64 MLP on it."""
        return (not any(policy is not None and is_set(self) for _, is_set, _, _, _, policy in _STAGES)
                and self.get_property("step_n_one_launch") == 1 and self.get_property("f64") == 0 and self.obs_dim % 4 == 0 and self.obs_dim <= 88
                and params.obs_dim == self.obs_dim and params.act_dim == self.act_dim and params.hidden == 64)

    def step_act_inplace(self, actions, params, noise, value_out, action_out, logp_out, obs_out=None, rew_out=None, done_out=None,
                         timeout_out=None):
        """step_inplace + Policy.act on the new observations in ONE launch (solorl_step_act): value_out [N] or [N,1], action_out [N,A] =
        mean + exp(logstd) * noise (noise [N,A] or None), logp_out [N] or [N,1] -- e.g. the NEXT step's rollout-storage rows.
        ``timeout_out`` as step_inplace's (still one launch)."""
        self._no_policy_tail("step_act_inplace")
        a = self._raw("actions", actions, (self.nenvs, self.act_dim))
        o, r, d, po, pr, pd = self._outputs((), (self._obs, self._rew, self._done), obs_out, rew_out, done_out)
        ic, info = self._info_block(self._info_c, self._info, self._info_alt, timeout_out, ())
        pv = self._per_env("value_out", value_out, ())
        pa = self._raw("action_out", action_out, (self.nenvs, self.act_dim))
        pl = self._per_env("logp_out", logp_out, ())
        pn = C.c_void_p(0) if noise is None else self._raw("noise", noise, (self.nenvs, self.act_dim))
        self._steps_issued += 1
        applied = self._before_step(actions)
        if applied is not actions:
            a = C.c_void_p(applied.data_ptr())
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_step_act(self._h, a, po, pr, pd, C.byref(ic), C.byref(params), pn, pv, pa, pl, self._stream()))
        self._after_step(o, o, r, d, actions, tail=True)
        return o, r, d, info

    def _k_rows(self, K):
        """Engine-owned output rows [K, N, ...] and their info block (every per-step field [K, N], applied torques [K, N, A] when
        recorded, ep_stats shared with step()), allocated at the first call with this K."""
        b = self._kbuf.get(K)
        if b is None or (b["tau"] is None) != (self._tau is None):
            N, kw = self.nenvs, dict(device=self.device)
            # (empty, not zeros: every step writes every field of every env, and a fill would be one more launch in a captured graph)
            info = {k: torch.empty((K, N), dtype=v.dtype, **kw) for k, v in self._info.items()}
            tau = None if self._tau is None else torch.empty((K, N, self.act_dim), dtype=torch.float32, **kw)
            if tau is not None:
                info["applied_torque"] = tau
            c = InfoSoA(ep_stats=self._ep_stats.data_ptr(), applied_torque=None if tau is None else tau.data_ptr(),
                        **{k: info[k].data_ptr() for k in _INFO_KEYS})
            b = dict(obs=None, info=info, tau=tau, c=c, alt={})      # alt: as _info_alt, for this K's block
            self._kbuf[K] = b
        return b

    def _rows_out(self, b, K, obs_out, rew_out, done_out):
        if b["obs"] is None and (obs_out is None or rew_out is None or done_out is None):      # (engine-owned rows: on first use only)
            kw = dict(device=self.device)
            b.update(obs=torch.empty((K, self.nenvs, self.obs_dim), dtype=torch.float32, **kw), rew=torch.empty((K, self.nenvs), dtype=torch.float32, **kw),
                     done=torch.empty((K, self.nenvs), dtype=torch.uint8, **kw))
        return self._outputs((K,), (b["obs"], b.get("rew"), b.get("done")), obs_out, rew_out, done_out)

    def step_n(self, actions):
        """K control steps (include/solorl.h solorl_step_n; one launch where get_property("step_n_one_launch") is 1): actions [K, N, A]
        -> (obs [K, N, O], reward [K, N, 1], done [K, N] float, infos: dict of per-step [K, N] tensors, "done" among them)."""
        if actions.dim() != 3 or actions.shape[1:] != (self.nenvs, self.act_dim) or actions.shape[0] < 1:
            raise AssertionError("actions must be [K, %d, %d]" % (self.nenvs, self.act_dim))
        a = actions.detach().to(device=self.device, dtype=torch.float32).contiguous()
        o, r, d, info = self.step_n_inplace(a)
        t = {k: v.clone() for k, v in info.items()}
        t["done"] = d.clone()
        return o.clone(), r.clone().unsqueeze(-1), t["done"].float(), t

    def step_n_inplace(self, actions, obs_out=None, rew_out=None, done_out=None, timeout_out=None):
        """step_inplace for K steps: actions [K, N, A] (float32, contiguous, on this device); returns views of engine-owned rows
        (overwritten by the next call with the same K) -- or writes observations [K, N, O] / rewards [K, N] or [K, N, 1] / done flags
        (uint8 [K, N]) / timeout flags (``timeout_out``: uint8 [K, N] or [K, N, 1]) straight into caller-owned tensors such as
        rollout-storage rows.  Host-side checks only, capturable."""
        self._refuse("step_n", k_step=True)
        K = int(actions.shape[0]) if actions.dim() == 3 else 0
        if K < 1:
            raise AssertionError("actions must be [K, %d, %d] with K >= 1" % (self.nenvs, self.act_dim))
        pa = self._raw("actions", actions, (K, self.nenvs, self.act_dim))
        b = self._k_rows(K)
        o, r, d, po, pr, pd = self._rows_out(b, K, obs_out, rew_out, done_out)
        ic, info = self._info_block(b["c"], b["info"], b["alt"], timeout_out, (K,))
        self._steps_issued += K
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_step_n(self._h, K, pa, po, pr, pd, C.byref(ic), self._stream()))
        if self._norm is not None:                      # one call for the window's K rows
            self._normalize(o, r, d, K)
        return o, r, d, info

    def rollout_supported(self, params):
        """solorl_rollout (K closed-loop steps in one launch) on this handle: the prerequisites of solorl_step_act, and no perturbation
        set (kicks come between two step launches), no reward shaping set (its launch comes behind every step launch) and neither
        observation noise nor actuation set (their launches stand behind and in front of every step launch)."""
        return not any(between is not None and is_set(self) for _, is_set, _, between, _, _ in _STAGES) and self.step_act_supported(params)

    def rollout_inplace(self, actions, params, noise, value_out, logp_out, obs_out=None, rew_out=None, done_out=None, policy_after_last=False,
                        timeout_out=None):
        """K closed-loop steps in one launch (solorl_rollout), in rollout-storage rows: actions [K (+1), N, A] -- row 0 drives the
        first step, rows 1.. are written by the policy on the observations the steps produce (row K too with policy_after_last: the
        first action of the next window); noise [K (+1), N, A] or None (actions = the mean); value_out / logp_out [K (+1), N] or
        [K (+1), N, 1], rows from 1 written; obs_out [K, N, O], rew_out [K, N] or [K, N, 1], done_out uint8 [K, N] and timeout_out
        uint8 [K, N] or [K, N, 1] as step_n_inplace."""
        self._refuse("rollout_inplace", tail=True)
        self._refuse("rollout_inplace", k_step=True)
        pal = 1 if policy_after_last else 0
        R = int(actions.shape[0]) if actions.dim() == 3 else 0
        K = R - pal
        if K < 1:
            raise AssertionError("actions must be [K%s, %d, %d] with K >= 1" % (" + 1" if pal else "", self.nenvs, self.act_dim))
        pa = self._raw("actions", actions, (R, self.nenvs, self.act_dim))
        pn = C.c_void_p(0) if noise is None else self._raw("noise", noise, (R, self.nenvs, self.act_dim))
        pv, pl = self._per_env("value_out", value_out, (R,)), self._per_env("logp_out", logp_out, (R,))
        b = self._k_rows(K)
        o, r, d, po, pr, pd = self._rows_out(b, K, obs_out, rew_out, done_out)
        ic, info = self._info_block(b["c"], b["info"], b["alt"], timeout_out, (K,))
        self._steps_issued += K
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_rollout(self._h, K, pa, po, pr, pd, C.byref(ic), C.byref(params), pn, pv, pl, pal, self._stream()))
        if self._norm_ret:                              # one call for the window's K rows, after the window
            self._normalize(o, r, d, K)
        return o, r, d, info

    def get_observation(self):
        """The clean observation rows; with velocity commands the current command words are appended (by torch ops)"""
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_get_observation(self._h, C.c_void_p(self._obs_engine.data_ptr()), self._stream()))
        if self._cmd is not None:
            return torch.cat([self._obs_engine, self._command_words()], dim=1)
        return self._obs.clone()

    def episode_stat_sums(self, reset=True):
        """Device tensor [SOLORL_EPSTAT_FIELDS]: the accumulators summed over this handle's envs (all-reduce it across
        ranks before dividing by field 0)."""
        tot = self._ep_stats.sum(dim=1)
        if reset:
            if self._term_eps is not None:              # termination_stats() counts finished episodes from this block: keep what is zeroed
                self._term_eps[0] += self._ep_stats[0].sum(dtype=torch.float64) - self._term_eps[1]
                self._term_eps[1] = 0.0
            self._ep_stats.zero_()
        return tot

    def episode_stats(self, reset=True):
        """Statistics of the episodes finished since the last call, reduced on the device from the engine's
        per-env accumulators (every step counts, nothing is sampled): the quantities the reference collects by
        iterating N info dicts per step (agents/ppo/train.py:90-100) -- means of info['episode_reward'] (the LAST
        step's reward, baseEnv.py:65), info['episode_length'], info['success'] and the info['dr/*'] sums over the
        finished episodes -- plus their count.  One small device->host copy; ``reset`` zeroes the accumulators."""
        tot = self.episode_stat_sums(reset).tolist()
        n = tot[0]
        out = {"episodes": int(n), "nan_resets": int(tot[9])}
        for k in range(1, 9):
            out[EPSTAT_NAMES[k]] = (tot[k] / n) if n > 0 else float("nan")
        return out

    def record_applied_torque(self):
        """Every step also writes the joint torques it applied (after the clip / PD law, solo.py:224-259) into the returned [N, A]
        tensor (overwritten by the next step).  Must be enabled before the first step (or with the constructor's
        ``applied_torque=True``): the destination is a kernel argument, so a rollout or bench graph captured earlier would keep
        replaying without it -- enabling it late raises instead of being silently ignored by those graphs."""
        if self._tau is None:
            if self._steps_issued:
                raise _native.SoloRLError("record_applied_torque() after %d steps: step launches (and any HIP graph captured from them) already "
                                          "carry a NULL applied_torque pointer; construct the env with applied_torque=True" % self._steps_issued)
            self._tau = torch.zeros((self.nenvs, self.act_dim), dtype=torch.float32, device=self.device)
            self._info_c.applied_torque = self._tau.data_ptr()
        return self._tau

    def increment_curriculum(self, value=1.0):
        _native.check(self.L.solorl_increment_curriculum(self._h, float(value)))

    def get_property(self, name):
        """Read-only handle properties (include/solorl.h solorl_get_property): lanes_per_env, sweep_variant, max_contacts,
        max_limit_rows, f64, step_n_one_launch, helper_wave"""
        v = C.c_double()
        _native.check(self.L.solorl_get_property(self._h, name.encode(), C.byref(v)))
        return v.value

    def get_state(self, i=0):
        s = EnvState()
        _native.check(self.L.solorl_get_state(self._h, int(i), C.byref(s)))
        return s

    def set_state(self, i, s):
        _native.check(self.L.solorl_set_state(self._h, int(i), C.byref(s)))

    # ---- the whole batch's state on the device (include/solorl.h solorl_get_states / solorl_set_states / solorl_reset_masked):
    # one launch each on the current stream, no host synchronisation -- capturable in a HIP graph
    def _mask(self, mask):
        """None, or a [N] torch.bool / torch.uint8 tensor on this device -> (tensor kept alive for the call, pointer)"""
        return mask_arg(mask, self.nenvs, self.device)

    def _rows(self, name, states):
        if not isinstance(states, StateBatch):
            raise AssertionError("%s must be a StateBatch" % name)
        d = states.data
        if not (d.is_cuda and d.device == self.device and d.shape[0] == self.nenvs):
            raise AssertionError("%s must hold %d rows on %s, got %d on %s" % (name, self.nenvs, self.device, d.shape[0], d.device))
        return C.c_void_p(d.data_ptr())

    def get_states(self, mask=None, out=None):
        """The state of every env (row i = env i) as a StateBatch on this device.  ``mask``: rows of unselected envs are left as they
        are in ``out`` (zeros in a fresh one)."""
        if out is None:
            out = StateBatch(self.nenvs, self.device)
        m, pm = self._mask(mask)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_get_states(self._h, pm, self._rows("out", out), self._stream()))
        return out

    def get_kinematics(self, mask=None, states=None, out=None):
        """Link poses, support points of the collision primitives with their velocities and normal forces, centre of mass, energy and
        momentum of every env (solorl_amd/kinematics.py KinBatch; include/solorl.h solorl_kinematics), on the current stream.
        ``states``: rows to use instead of the handle's current state; without it ``get_states(mask)`` fills an engine-owned StateBatch
        (allocated at the first call, so a HIP graph captured after a warm-up call keeps using it)."""
        from .kinematics import kinematics
        return self._row_query(kinematics, "_kin_states", mask, states, out)

    def get_dynamics(self, mask=None, states=None, out=None):
        """Joint-space mass matrix, bias and gravity forces, foot Jacobians with their Jdot v and foot points of every env
        (solorl_amd/dyn_tensors.py DynBatch; include/solorl.h solorl_dynamics), on the current stream.  ``states``: rows to use instead of
        the handle's current state; without it ``get_states(mask)`` fills an engine-owned StateBatch (allocated at the first call, so a
        HIP graph captured after a warm-up call keeps using it)."""
        from .dyn_tensors import dynamics
        return self._row_query(dynamics, "_dyn_states", mask, states, out)

    def _row_query(self, call, own, mask, states, out):
        """``call`` (kinematics or dynamics) on ``states``, or on the handle's current state read into the engine-owned StateBatch
        kept in attribute ``own`` (one per query: a graph captured around one call does not depend on the other's rows)"""
        if states is None:
            if getattr(self, own) is None:
                setattr(self, own, StateBatch(self.nenvs, self.device))
            states = self.get_states(mask, out=getattr(self, own))
        else:
            self._rows("states", states)
        m, _ = self._mask(mask)
        return call(self.cfg, states, m, out)

    def set_states(self, states, mask=None, fields="all"):
        """Writes the member groups ``fields`` (a name, an iterable of names -- pose, vel, joint_pos, joint_vel, contact, history, task,
        counters, all -- or an int of SOLORL_SF_* bits) of the selected envs from ``states``; everything else stays.  Nothing is derived
        on a partial write except the engine's previous-xy from ``pos`` (include/solorl.h): teleporting a pointgoal env needs
        ``potential`` rewritten too.  Without mask and with all groups it also counts as the handle's reset."""
        m, pm = self._mask(mask)
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_set_states(self._h, pm, self._rows("states", states), field_bits(fields), self._stream()))

    def reset_masked(self, mask):
        """reset() for the envs selected by ``mask`` only (each draws from its own Philox counter, as at a full or an in-step reset)
        -> obs [N, O]: the rows of the selected envs are their reset observations, every other row is that env's CURRENT observation
        (the observation buffer is refilled by solorl_get_observation first)."""
        m, pm = self._mask(mask)
        if m is None:
            raise AssertionError("reset_masked needs a mask (reset() resets every env)")
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_get_observation(self._h, C.c_void_p(self._obs_engine.data_ptr()), self._stream()))
            _native.check(self.L.solorl_reset_masked(self._h, pm, C.c_void_p(self._obs_engine.data_ptr()), self._stream()))
        self._randomize(self._obs_engine, m)
        if self._act is not None:                       # the selected envs start an episode with their next action
            self._act_restart.bitwise_or_(m.ne(0).to(torch.uint8))
        if self._cmd is not None:                       # every row with the command it holds; the selected ones are rewritten below
            self._obs.copy_(torch.cat([self._obs_engine, self._command_words()], dim=1))
        c = self._clean_rows(self._obs_engine)
        if c is not self._obs_engine:                   # every row before the noise, for the critic rows
            c.copy_(self._obs_engine)
        self._noise(self._obs_engine, m)                # the rows the engine has just written: the selected ones
        self._commands(self._obs, m, mask=m)            # the selected envs draw a command; no other row is touched
        self._critic_rows(c)                            # every row: the unselected ones describe their current state too
        if self._shape_mem is not None:                 # the selected envs start an episode (its sums so far are dropped, not counted)
            self._shape_mem.data.masked_fill_(m.bool().unsqueeze(-1), 0.0)
        if self._norm is not None:
            sel = m.bool()
            self._norm.ret.masked_fill_(sel, 0.0)       # a reset env starts a new return (running_mean_std.py:105)
            if self._norm_obs:                           # the selected rows as a reset() gives them, without an update; the others stay raw
                return torch.where(sel.unsqueeze(-1), self._norm.obs(self._obs, 1, False, out=torch.empty_like(self._obs)), self._obs)
        return self._obs.clone()

    def push(self, dv, mask=None):
        """Kicks the base velocity of the selected envs: ``dv`` [N, 3] is added to the linear velocity, [N, 6] to (linear, angular),
        world frame.  get_states -> add -> set_states(fields = vel) on an engine-owned StateBatch (allocated at the first call, so a
        HIP graph captured after a warm-up call keeps using it); nothing but the two velocities is written."""
        if dv.dim() != 2 or dv.shape[0] != self.nenvs or dv.shape[1] not in (3, 6) or dv.device != self.device:
            raise AssertionError("dv must be [%d, 3] or [%d, 6] on %s" % (self.nenvs, self.nenvs, self.device))
        if self._push_states is None:
            self._push_states = StateBatch(self.nenvs, self.device)
        s = self._push_states
        self.get_states(mask, out=s)
        s.lin_vel.add_(dv[:, :3])
        if dv.shape[1] == 6:
            s.ang_vel.add_(dv[:, 3:])
        self.set_states(s, mask, SF_VEL)

    def close(self):
        if not self.closed and getattr(self, "_h", None):
            self.L.solorl_destroy(self._h)
            self._h = None
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


for _guard in sorted({g for g, _, _, between, _, _ in _STAGES if between is not None}):       # _no_kicks(name), _no_shaping, _no_channel ...
    setattr(SoloVecEnv, "_no_" + _guard, lambda self, name, _g=_guard: self._refuse(name, k_step=True, guard=_g))


def make_vec_envs(config, num_envs, env_constructor=None, gamma=0.99, device=None, training=True, seed=1,
                  env_id_offset=0, norm_obs=False, norm_ret=False, clipob=10., cliprew=10., epsilon=1e-8,
                  push_interval=None, push_max_vel=0.0, push_max_yaw_rate=0.0, reward_shaping=None,
                  obs_noise=None, action_delay=None, motor_gain_range=0.0, commands=None, termination=None, reset_randomization=None,
                  critic_obs=None):
    """Signature of agents/ppo/envs.py:14.  ``env_constructor`` (the per-process gym env class of the
    reference) is accepted for call-site compatibility and ignored.  ``norm_obs`` / ``norm_ret`` are VecNormalize's ``ob`` /
    ``ret`` (agents/running_mean_std.py:79; the reference's launcher passes False, False, and so do the defaults here) with its
    ``clipob``, ``cliprew``, ``epsilon``; ``gamma`` is the discount of its return accumulator and means something with ``norm_ret``.
    ``training=False`` is its eval() (agents/ppo/envs.py:27-28).
    ``push_interval`` (an int or a (lo, hi) pair of control steps; None = no kicks, and nothing is allocated or launched): random kicks of
    up to ``push_max_vel`` m/s on the base's world x and y velocity and ``push_max_yaw_rate`` rad/s on its yaw rate, in front of every
    step (SoloVecEnv.set_perturbation).
    ``reward_shaping`` (a dict with ``weights`` and the parameters as further keys, as configs/shaping_walk12.yaml holds it; None = no
    shaping, and nothing is allocated or launched): shaped reward terms behind every step (SoloVecEnv.set_reward_shaping).
    ``obs_noise`` (a dict of half-widths per observation group, or a noise file's dict with ``groups`` and ``history`` as
    configs/noise_solo.yaml holds it, or an [obs_dim] vector; None = clean observations): uniform sensor noise on every observation
    (SoloVecEnv.set_obs_noise).  ``action_delay`` (an int or a (lo, hi) pair of control steps within 0..4; None = none) and
    ``motor_gain_range`` (each joint's action is scaled by 1 + U(-g, g), drawn per env and episode; 0 = exact): actuation latency and
    motor gain error in front of every step (SoloVecEnv.set_actuation).  Off, nothing is allocated or launched.
    ``commands`` (a dict with ``lin_vel_x``, ``lin_vel_y``, ``yaw_rate`` as [lo, hi] pairs, ``interval``, ``zero_prob``, ``min_lin_norm``,
    ``obs_scale``, as configs/commands_walk12.yaml holds it; None = no commands, and nothing is allocated or launched): per-env velocity
    commands, three more observation words, and the tracking terms of ``reward_shaping`` against each env's own command.
    ``termination`` (a dict with ``base_height``, ``max_tilt_deg``, ``contacts``, ``contact_force_min``, ``joint_limits``, ``min_steps``,
    ``terminal_reward``, as configs/termination_walk12.yaml holds it; None = the engine's own endings only, and nothing is allocated or
    launched): early termination rules behind every step (SoloVecEnv.set_termination).
    ``reset_randomization`` (a dict with ``joint_pos``, ``joint_vel``, ``lin_vel``, ``ang_vel``, ``yaw``, ``roll``, ``pitch``, ``clearance``,
    ``place_on_ground``, as configs/reset_walk12.yaml holds it; None = the engine's own snapshots, and nothing is allocated or launched):
    randomised initial states behind every reset (SoloVecEnv.set_reset_randomization).
    ``critic_obs`` (True, or a dict of scale overrides per group of privileged words as configs/critic_walk12.yaml holds it; None = no
    critic rows, and nothing is allocated or launched): privileged critic rows behind every step and reset (SoloVecEnv.last_critic_obs)."""
    envs = SoloVecEnv(config, num_envs, device=device, seed=seed, env_id_offset=env_id_offset, norm_obs=norm_obs, norm_ret=norm_ret,
                      clipob=clipob, cliprew=cliprew, gamma=gamma, epsilon=epsilon, commands=commands, critic_obs=critic_obs)
    if push_interval is not None:
        envs.set_perturbation(push_interval, (push_max_vel, push_max_vel, 0.0), (0.0, 0.0, push_max_yaw_rate))
    if reward_shaping is not None:
        rs = dict(reward_shaping)
        weights = rs.pop("weights", None)
        if not isinstance(weights, dict):
            raise ValueError("reward_shaping needs a `weights` mapping of term name -> weight")
        envs.set_reward_shaping(weights, **rs)
    if obs_noise is not None:
        envs.set_obs_noise(obs_noise)
    if action_delay is not None or motor_gain_range:
        envs.set_actuation(action_delay, motor_gain_range)
    if termination is not None:
        from .termination import rules_from_dict
        envs.set_termination(**rules_from_dict(termination))
    if reset_randomization is not None:
        from .reset_random import ranges_from_dict
        envs.set_reset_randomization(**ranges_from_dict(reset_randomization))
    if not training:
        envs.eval()
    return envs
