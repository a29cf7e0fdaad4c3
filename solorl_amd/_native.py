"""ctypes binding of the C ABI (include/solorl.h).  No CPU fallback: if the HIP library is
missing or no GPU is present every entry point raises (the product path never touches oracle/)."""
import ctypes as C
import os

# torch must be imported BEFORE the engine is dlopen'ed: both depend on libamdhip64.so.7 and the
# first copy loaded wins; torch's bundled HIP runtime has to be that copy or device init fails.
import torch  # noqa: F401

from .config import SoloConfig, EnvState, InfoSoA, ABI_VERSION

_LIB = None
LIB_PATH = os.environ.get("SOLORL_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libsolorl_hip.so")   # SOLORL_LIB: dev A/B builds

# every symbol include/solorl.h declares
SYMBOLS = ("solorl_default_config", "solorl_create", "solorl_destroy", "solorl_dims", "solorl_reset", "solorl_step",
           "solorl_get_observation", "solorl_increment_curriculum", "solorl_get_state", "solorl_set_state", "solorl_get_property",
           "solorl_compute_returns", "solorl_compute_returns_tl", "solorl_ppo_loss", "solorl_policy_act", "solorl_ppo_grad_stage1", "solorl_ppo_grad_stage2", "solorl_ppo_grad_count", "solorl_ppo_clip_adam", "solorl_last_error", "solorl_version",
           "solorl_abi_version", "solorl_step_act", "solorl_ppo_scratch_count", "solorl_step_n", "solorl_rollout",
           "solorl_get_states", "solorl_set_states", "solorl_reset_masked",
           "solorl_set_perturbation", "solorl_perturb", "solorl_get_perturbation",
           "solorl_norm_scratch_count", "solorl_normalize_obs", "solorl_normalize_rewards", "solorl_kinematics", "solorl_dynamics",
           "solorl_shape_reward", "solorl_obs_noise", "solorl_actuate", "solorl_commands", "solorl_shape_reward_cmd",
           "solorl_terminate", "solorl_randomize_reset", "solorl_restart_history", "solorl_critic_obs",
           "solorl_policy_act_critic", "solorl_ppo_grad_stage1_critic", "solorl_ppo_grad_stage2_critic", "solorl_ppo_grad_count2", "solorl_ppo_scratch_count2",
           "solorl_policy_act_w", "solorl_ppo_grad_stage1_w", "solorl_ppo_grad_stage2_w", "solorl_ppo_clip_adam_w",
           "solorl_ppo_grad_stage1_kl", "solorl_ppo_clip_adam_kl")

POLICY_MAX_WIDTH = 128                      # SOLORL_POLICY_MAX_WIDTH


class PolicyParams(C.Structure):            # solorl_policy_params
    _fields_ = [("obs_dim", C.c_int), ("act_dim", C.c_int), ("hidden", C.c_int), ("critic_obs_dim", C.c_int)] + [
        (n, C.c_void_p) for n in ("critic_w0", "critic_b0", "critic_w1", "critic_b1", "critic_w2", "critic_b2", "actor_w0", "actor_b0",
                                  "actor_w1", "actor_b1", "mean_w", "mean_b", "logstd")]


class PpoBatch(C.Structure):                # solorl_ppo_batch
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "old_logp", "adv", "vpred", "ret", "perm", "offset")] + [
        ("m", C.c_int), ("clipped_value", C.c_int), ("clip", C.c_float), ("value_coef", C.c_float)]


class PpoGrads(C.Structure):                # solorl_ppo_grads
    _fields_ = [(n, C.c_void_p) for n in ("critic_w0", "critic_b0", "critic_w1", "critic_b1", "critic_w2", "critic_b2", "actor_w0", "actor_b0",
                                          "actor_w1", "actor_b1", "mean_w", "mean_b", "logstd", "loss_sums", "logstd_sum", "scratch")] + [
        ("entropy_coef", C.c_float), ("reserved0", C.c_float)]


class AdamState(C.Structure):               # solorl_adam_state
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("step", C.c_void_p), ("lr", C.c_void_p), ("offset", C.c_void_p),
                ("offset_increment", C.c_int64), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("max_grad_norm", C.c_float), ("grad_scale", C.c_float)]


class KlControl(C.Structure):               # solorl_kl_control
    _fields_ = [("diag", C.c_void_p), ("m", C.c_int), ("desired_kl", C.c_float), ("lr_factor", C.c_float), ("lr_min", C.c_float),
                ("lr_max", C.c_float), ("target_kl", C.c_float), ("lr", C.c_void_p), ("state", C.c_void_p), ("log", C.c_void_p),
                ("log_capacity", C.c_int)]


class PpoStage1(C.Structure):               # solorl_ppo_stage1
    _fields_ = [(n, C.c_void_p) for n in ("xt0", "c_xt1", "c_xt2", "c_g1", "c_g2", "c_gh", "a_xt1", "a_xt2", "a_g1", "a_g2", "a_gh", "partials")]


class Perturbation(C.Structure):            # solorl_perturbation
    _fields_ = [("interval_min", C.c_int32), ("interval_max", C.c_int32), ("max_lin_vel", C.c_double * 3), ("max_ang_vel", C.c_double * 3)]


DELAY_MAX = 4                               # SOLORL_DELAY_MAX


class Actuation(C.Structure):               # solorl_actuation
    _fields_ = [("seed", C.c_uint64), ("env_id_offset", C.c_int64), ("act_dim", C.c_int32), ("delay_min", C.c_int32), ("delay_max", C.c_int32),
                ("reserved", C.c_int32), ("gain_range", C.c_double)]


class EnvActuator(C.Structure):             # solorl_env_actuator
    _fields_ = [("buf", (C.c_float * 12) * DELAY_MAX), ("gain", C.c_float * 12), ("latency", C.c_int32), ("fill", C.c_int32),
                ("episodes", C.c_uint32), ("reserved", C.c_int32)]


class CommandParams(C.Structure):           # solorl_command_params
    _fields_ = [("seed", C.c_uint64), ("env_id_offset", C.c_int64), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("obs_scale", C.c_double * 3),
                ("zero_prob", C.c_double), ("min_lin_norm", C.c_double), ("interval_min", C.c_int32), ("interval_max", C.c_int32),
                ("obs_dim", C.c_int32), ("reserved", C.c_int32)]


class EnvCommand(C.Structure):              # solorl_env_command
    _fields_ = [("cmd", C.c_double * 3), ("countdown", C.c_int32), ("draws", C.c_uint32)]


TERM_RULES = 4                              # SOLORL_TERM_RULES


class Termination(C.Structure):             # solorl_termination
    _fields_ = [("rules", C.c_uint32), ("min_steps", C.c_int32), ("contact_prims", C.c_uint32), ("reserved", C.c_int32), ("min_height", C.c_double),
                ("min_up_z", C.c_double), ("contact_force_min", C.c_double), ("joint_lo", C.c_double * 12), ("joint_hi", C.c_double * 12),
                ("terminal_reward", C.c_double)]


class ResetRandomization(C.Structure):      # solorl_reset_randomization
    _fields_ = [("seed", C.c_uint64), ("env_id_offset", C.c_int64), ("joint_pos", C.c_double * 12), ("joint_vel", C.c_double * 12),
                ("lin_vel", C.c_double * 3), ("ang_vel", C.c_double * 3), ("yaw", C.c_double), ("roll", C.c_double), ("pitch", C.c_double),
                ("clearance", C.c_double), ("place_on_ground", C.c_int32), ("reserved", C.c_int32)]


CRITIC_PRIV = 20                            # SOLORL_CRITIC_PRIV


class CriticParams(C.Structure):            # solorl_critic_params
    _fields_ = [("scale", C.c_double * CRITIC_PRIV), ("obs_dim", C.c_int32), ("reserved", C.c_int32)]


class SoloRLError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SoloRLError("HIP engine not built: %s missing (run `python -m solorl_amd.build`); "
                              "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.solorl_last_error.restype = C.c_char_p
        L.solorl_version.restype = C.c_char_p
        L.solorl_default_config.argtypes = [C.POINTER(SoloConfig), C.c_int, C.c_int]
        L.solorl_create.argtypes = [C.POINTER(SoloConfig), C.c_int, C.c_int, C.c_uint64, C.c_int64, C.POINTER(C.c_void_p)]
        L.solorl_destroy.argtypes = [C.c_void_p]
        L.solorl_dims.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.solorl_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InfoSoA), C.c_void_p]
        L.solorl_get_observation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_step_act.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InfoSoA), C.POINTER(PolicyParams), C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_step_n.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InfoSoA), C.c_void_p]
        L.solorl_rollout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(InfoSoA), C.POINTER(PolicyParams),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_increment_curriculum.argtypes = [C.c_void_p, C.c_double]
        L.solorl_get_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(EnvState)]
        L.solorl_set_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(EnvState)]
        # batched state access: mask, rows and observations are device pointers
        L.solorl_get_states.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_set_states.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.solorl_reset_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for f in (L.solorl_get_states, L.solorl_set_states, L.solorl_reset_masked):
            f.restype = C.c_int
        # device-side kicks: the struct is a host pointer (None = off), kick_out / countdown_out / kicks_out are device pointers
        L.solorl_set_perturbation.argtypes = [C.c_void_p, C.POINTER(Perturbation)]
        L.solorl_perturb.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_get_perturbation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for f in (L.solorl_set_perturbation, L.solorl_perturb, L.solorl_get_perturbation):
            f.restype = C.c_int
        L.solorl_get_property.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        L.solorl_ppo_loss.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p]
        L.solorl_compute_returns.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                             C.c_float, C.c_float, C.c_int, C.c_void_p]
        # the same with the timeout flags [T*N] (uint8) in front of next_value
        L.solorl_compute_returns_tl.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]
        L.solorl_compute_returns_tl.restype = C.c_int
        L.solorl_policy_act.argtypes = [C.POINTER(PolicyParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_ppo_grad_stage1.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoBatch), C.POINTER(PpoStage1), C.c_int, C.c_void_p]
        L.solorl_ppo_grad_stage2.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoStage1), C.c_int, C.POINTER(PpoGrads), C.c_int, C.c_void_p]
        L.solorl_ppo_grad_count.argtypes = [C.c_int, C.c_int]
        L.solorl_ppo_scratch_count.argtypes = [C.c_int, C.c_int, C.c_int]
        L.solorl_ppo_scratch_count.restype = C.c_int
        # the asymmetric policy (critic_obs_dim != 0): the critic's rows beside the actor's
        L.solorl_policy_act_critic.argtypes = [C.POINTER(PolicyParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_ppo_grad_stage1_critic.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoBatch), C.c_void_p, C.POINTER(PpoStage1), C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_ppo_grad_stage2_critic.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoStage1), C.c_void_p, C.c_int, C.POINTER(PpoGrads), C.c_int, C.c_void_p]
        L.solorl_ppo_grad_count2.argtypes = [C.c_int, C.c_int, C.c_int]
        L.solorl_ppo_scratch_count2.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.solorl_ppo_clip_adam.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoGrads), C.POINTER(AdamState), C.c_int, C.c_void_p]
        # the width-generic family: the _critic argument lists, the critic's arrays NULL for a symmetric policy
        L.solorl_policy_act_w.argtypes = L.solorl_policy_act_critic.argtypes
        L.solorl_ppo_grad_stage1_w.argtypes = L.solorl_ppo_grad_stage1_critic.argtypes
        L.solorl_ppo_grad_stage2_w.argtypes = L.solorl_ppo_grad_stage2_critic.argtypes
        L.solorl_ppo_clip_adam_w.argtypes = L.solorl_ppo_clip_adam.argtypes
        # KL control: one pair for the three kernel families (generic: the _w kernels; the critic's arrays NULL for a symmetric policy)
        L.solorl_ppo_grad_stage1_kl.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoBatch), C.c_void_p, C.POINTER(PpoStage1), C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_int, C.c_void_p]
        L.solorl_ppo_clip_adam_kl.argtypes = [C.POINTER(PolicyParams), C.POINTER(PpoGrads), C.POINTER(AdamState), C.POINTER(KlControl), C.c_int, C.c_int,
                                              C.c_void_p]
        # running normalisation: stats / ret / scratch are device pointers to doubles
        L.solorl_norm_scratch_count.argtypes = [C.c_int, C.c_int, C.c_int]
        L.solorl_normalize_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                           C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_normalize_rewards.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                               C.c_double, C.c_void_p, C.c_int, C.c_void_p]
        for f in (L.solorl_norm_scratch_count, L.solorl_normalize_obs, L.solorl_normalize_rewards):
            f.restype = C.c_int
        # derived quantities of state rows: states, mask and out are device pointers
        L.solorl_kinematics.argtypes = [C.POINTER(SoloConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_kinematics.restype = C.c_int
        L.solorl_dynamics.argtypes = [C.POINTER(SoloConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_dynamics.restype = C.c_int
        # shaped reward terms (shaping.py holds the mirrors): cfg and params are host structs, everything else a device pointer
        L.solorl_shape_reward.argtypes = [C.POINTER(SoloConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_shape_reward.restype = C.c_int
        # observation noise and actuation (channel.py): handle-free; params is a host struct, every array a device pointer
        L.solorl_obs_noise.argtypes = [C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_actuate.argtypes = [C.POINTER(Actuation), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_obs_noise.restype = L.solorl_actuate.restype = C.c_int
        # velocity commands (command.py): handle-free; params is a host struct, every array a device pointer.  solorl_shape_reward_cmd is
        # solorl_shape_reward with the command rows in front of device_id
        L.solorl_commands.argtypes = [C.POINTER(CommandParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p]
        L.solorl_shape_reward_cmd.argtypes = L.solorl_shape_reward.argtypes[:11] + [C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_commands.restype = L.solorl_shape_reward_cmd.restype = C.c_int
        # early termination (termination.py): handle-free; cfg, params and the info block are host structs, every array a device pointer
        L.solorl_terminate.argtypes = [C.POINTER(SoloConfig), C.POINTER(Termination), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(InfoSoA), C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_terminate.restype = C.c_int
        # randomised initial states (reset_random.py): the row query is handle-free (cfg and params are host structs, rows, mask and count
        # device pointers); the history restart takes the handle, a device mask and the observation rows
        L.solorl_randomize_reset.argtypes = [C.POINTER(SoloConfig), C.POINTER(ResetRandomization), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_void_p]
        L.solorl_restart_history.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.solorl_randomize_reset.restype = L.solorl_restart_history.restype = C.c_int
        # privileged critic rows (critic_obs.py): handle-free; cfg and params are host structs, every array a device pointer
        L.solorl_critic_obs.argtypes = [C.POINTER(SoloConfig), C.POINTER(CriticParams), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.solorl_critic_obs.restype = C.c_int
        for s in SYMBOLS:
            getattr(L, s)
        # the ctypes mirrors in config.py / this file are written against one layout of include/solorl.h's structs
        if L.solorl_abi_version() != ABI_VERSION:
            raise SoloRLError("%s was built for ABI version %d, this binding is written for %d: rebuild (`python -m solorl_amd.build`)"
                              % (LIB_PATH, L.solorl_abi_version(), ABI_VERSION))
        _LIB = L
    return _LIB


def stream(device):
    """The caller's current HIP stream on `device`, as the C ABI takes it"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc):
    if rc != 0:
        raise SoloRLError("solorl error %d: %s" % (rc, lib().solorl_last_error().decode()))
