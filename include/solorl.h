/* solorl.h -- C ABI of the MI355X-native Solo8/Solo12 rollout engine.
 *
 * Drop-in boundary for the reference's vec-env layer.  Each entry point
 * replaces what the reference does through N worker processes and pickled Pipe messages:
 *
 *   solorl_create          <- agents/ppo/envs.py:14-30 (make_vec_envs), :66-89 (VecEnvWrapper.__init__
 *                             forking N `simple_worker`s, each building SoloBaseEnv(config):
 *                             baseEnv.py:7-40 -> solo.py:55-67)
 *   solorl_reset           <- agents/ppo/envs.py:97-100,198-200 -> baseEnv.py:70-82 (reset)
 *   solorl_step            <- agents/ppo/envs.py:91-95,189-196 -> :36-40 (worker: step + auto-reset)
 *                             -> baseEnv.py:42-68 (step)
 *   solorl_get_observation <- agents/ppo/envs.py:102-105,206-208 -> baseEnv.py:88-89
 *   solorl_dims            <- agents/ppo/envs.py:112-114 (get_spaces) -> baseEnv.py:20-28
 *   solorl_increment_curriculum <- agents/ppo/envs.py:125-127 (pointgoal: solo.py:332-334)
 *   solorl_compute_returns <- agents/ppo/storage.py:35-55 (OPBuffer.compute_returns: GAE / discounted returns;
 *                             400 sequential tiny torch ops per update in the reference)
 *   solorl_compute_returns_tl : the same with time-limit bootstrapping (no reference counterpart: its returns treat an episode the
 *                             time limit ended like a fall): a truncated step bootstraps from the value of the observation its
 *                             action was taken from, read from the timeout flags the step kernels write
 *   solorl_ppo_loss        <- agents/ppo/ppo.py:52-74 (clipped surrogate + clipped value loss) with the Gaussian
 *                             log-prob of agents/ppo/policy.py:51-58,171-173: ~60 elementwise torch kernels per mini-batch
 *   solorl_policy_act      <- agents/ppo/policy.py:33-49 (Policy.act on the MLPBase of :62-81): value, sampled action, log-prob
 *   solorl_ppo_grad_stage1 <- agents/ppo/ppo.py:46-74 for one mini-batch: storage.py:57-71 gather, policy.py:51-58
 *                             evaluate_actions, the clipped losses, and autograd's back-propagation down to every layer's
 *                             pre-activation gradient (what `loss.backward()` computes before the weight-gradient GEMMs)
 *   solorl_ppo_grad_stage2 <- the weight-gradient products of that backward pass, written into the parameters' gradients
 *   solorl_ppo_clip_adam   <- agents/ppo/ppo.py:75-77 (clip_grad_norm_ + optimizer.step) on the MLP's 13 parameter tensors
 *   solorl_step_act        <- agents/ppo/train.py:84-88: the rollout's pair `actor_critic.act(obs)` + `envs.step(action)` as ONE launch
 *                             (the policy is evaluated on each observation by the wavefront that has just produced it)
 *   solorl_step_n / solorl_rollout : K x solorl_step / solorl_step_act in one launch (no reference counterpart: the reference's
 *                             send-all / receive-all of agents/ppo/envs.py:91-95 is a barrier between every two steps)
 *   solorl_get_state / solorl_set_state / solorl_get_property : no reference counterpart (parity-test hooks, run records)
 *   solorl_get_states / solorl_set_states / solorl_reset_masked : the whole batch's state as ONE DEVICE array of solorl_env_state
 *                             rows, read and written by a kernel on the caller's stream (no reference counterpart: the reference
 *                             reaches an env's state only inside its worker process).  What pushes (kick the base velocity of every
 *                             env), starts from a chosen state distribution, branching one env into many, resetting a chosen subset,
 *                             saving / restoring a batch and logging a batch reduce to.  Row i is env i of the handle; a byte mask
 *                             selects envs, SOLORL_SF_* bits select member groups on write.  No host synchronisation: capturable.
 *   solorl_set_perturbation / solorl_perturb / solorl_get_perturbation : random base kicks at random intervals, drawn on the device from a
 *                             Philox stream per env and applied in place by one launch between two steps (no reference counterpart)
 *   solorl_normalize_obs / solorl_normalize_rewards <- agents/running_mean_std.py:73-127 (VecNormalize: _obfilt :109-116, the reward half
 *                             of step :98-105) with RunningMeanStd.update (:18-39), which agents/ppo/envs.py:25-26 wraps round the vec-env:
 *                             running statistics in caller-owned device memory, fp64, a fixed number of launches for any number of rows
 *   solorl_kinematics      <- what the reference asks PyBullet for per env (solo.py getLinkState / getContactPoints): link poses, support
 *                             points of the collision primitives with their velocities and normal forces, centre of mass, energy and
 *                             momentum of a whole batch of state rows, one launch
 *   solorl_dynamics        <- what the reference's MPC / WBC envs ask Pinocchio for and Isaac-style vec-envs expose as
 *                             jacobian / mass_matrix tensors: joint-space mass matrix, bias and gravity forces, foot Jacobians and their
 *                             Jdot v of a whole batch of state rows, one launch
 *   solorl_shape_reward    <- no reference counterpart (its reward is baseEnv.py's five terms): sixteen shaped reward terms -- base motion,
 *                             torques, joint acceleration, action rate, power, foot slip, clearance, contact force, air time, collisions,
 *                             command tracking -- of a whole batch of state rows added to the step's reward, one launch, with the
 *                             per-env memory these terms need in caller-owned device rows
 *   solorl_obs_noise / solorl_actuate : what stands between the policy and the engine in a randomised training run (no reference
 *                             counterpart): uniform sensor noise on observation rows, and actuation latency with a per-joint motor gain
 *                             error on action rows -- drawn on the device from a Philox stream per env, one launch each, handle-free
 *   solorl_commands / solorl_shape_reward_cmd : per-env velocity commands (no reference counterpart): drawn from ranges and resampled on
 *                             the device from a Philox stream per env, appended to the observation rows as three words, one launch,
 *                             handle-free; and the shaped reward's two tracking terms against each env's own command
 *   solorl_terminate       <- no reference counterpart (the reference ends an episode at the time limit, at a reached goal and at
 *                             pos.z < 0.05 only: baseEnv.py:162-180): early termination rules -- base height, tilt, contact of chosen
 *                             primitives, joint limits -- on a whole batch of state rows after a step, one launch, handle-free; it
 *                             sets done, the terminal reward and the episode statistics and leaves a mask for solorl_reset_masked
 *   solorl_randomize_reset / solorl_restart_history : randomised initial states (no reference counterpart: its reset is one fixed pose
 *                             and a random settle count): joint angles and velocities, base velocity and heading, roll and pitch of a
 *                             whole batch of state rows drawn on the device from a Philox stream per env, the robot placed on the
 *                             ground by the kinematics of the new pose, one launch, handle-free; and the handle's history restarted
 *                             from the state it holds, so that the first observation's delta words are exactly 0
 *   solorl_destroy        <- agents/ppo/envs.py:129-135 (close)
 *
 * Plain pointers and sizes only; no torch types.  All array arguments are DEVICE pointers
 * (HIP, the device the handle was created on); the engine never retains them past the stream
 * work of the call.  All work is enqueued on the `stream` argument (a hipStream_t passed as
 * void*; NULL = the null stream) and no entry point synchronises the host except
 * solorl_create/solorl_destroy/solorl_get_state/solorl_set_state/solorl_set_perturbation.
 *
 * Error convention: every function returns 0 on success or a negative code; the message is
 * available from solorl_last_error() (thread-local).  A per-env numeric failure (NaN/Inf state)
 * is NOT an error: the env is force-terminated, reset and counted in info.nan_reset.
 *
 * A handle is not thread-safe; one caller thread and one GPU per handle.
 */
#ifndef SOLORL_H
#define SOLORL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SOLORL_ROBOT_SOLO8 = 0, SOLORL_ROBOT_SOLO12 = 1 };
enum { SOLORL_TASK_STAND = 0, SOLORL_TASK_WALK = 1, SOLORL_TASK_POINTGOAL = 2 };
enum { SOLORL_CONTROL_TORQUE = 0, SOLORL_CONTROL_PD = 1 };
enum { SOLORL_PRECISION_F32 = 0, SOLORL_PRECISION_F64 = 1 };
enum { SOLORL_FRICTION_PYRAMID = 0, SOLORL_FRICTION_CONE = 1 };

/* Bumped whenever a struct of this header changes layout or meaning; solorl_abi_version() returns the value the library was built with
 * and a binding compares the two before its first call (a caller built against another layout would hand over short structs). */
#define SOLORL_ABI_VERSION 5

enum {
  SOLORL_OK = 0,
  SOLORL_ERR_INVALID = -1,   /* bad argument / config */
  SOLORL_ERR_NODEVICE = -2,  /* no usable HIP device */
  SOLORL_ERR_HIP = -3,       /* a HIP runtime call failed */
  SOLORL_ERR_STATE = -4      /* step() before reset() (reference baseEnv.py:43 assert) */
};

/* Task/robot/physics configuration: the YAML keys the reference reads in baseEnv.py:8-16,164
 * plus the Bullet parameters the reference leaves at PyBullet defaults. */
typedef struct solorl_config {
  int32_t robot;            /* SOLORL_ROBOT_*  (from model_urdf basename / `solo12: True`) */
  int32_t task;             /* SOLORL_TASK_*   (config 'task', baseEnv.py:11) */
  int32_t control;          /* SOLORL_CONTROL_* (config 'control', baseEnv.py:10; pd = pd/fpd/fixed_pd) */
  int32_t frame_skip;       /* config 'frame_skip' (default 4) */
  int32_t episode_length;   /* config 'episode_length' (baseEnv.py:164) */
  int32_t num_history_stack;/* config 'num_history_stack' (solo.py:48 deque(maxlen=h)): 0..4 (SOLORL_STATE_MAX_HISTORY) */
  int32_t hold_torque;      /* 0: torque acts on sub-step 1 only (Bullet clears it, K8); 1: held */
  int32_t use_urdf_inertia; /* 0: Bullet default box inertia from collision AABB (K2); 1: URDF tensor */
  int32_t solver_iterations;/* PGS iterations (PyBullet default 50, K7) */
  int32_t settle_min;       /* reset: K ~ U{settle_min .. settle_max} zero-torque control steps */
  int32_t settle_max;       /*        (baseEnv.py:79: randint(5,12) -> 5..11)                      */
  int32_t disable_termination; /* parity runs: never set done */
  int32_t precision;        /* SOLORL_PRECISION_*: arithmetic type of the HIP engine */
  int32_t use_treadmill;    /* config 'use_treadmill' (simulation.py:24-26,45-77): friction strip, see treadmill_* below */
  int32_t friction_model;   /* SOLORL_FRICTION_*: how the two friction rows of a contact are bounded by mu * normal impulse.
                             * PYRAMID: each row clamped to +-mu lambda_n on its own, Gauss-Seidel between the two (rounds 1-3).
                             * CONE: Bullet's implicit friction cone [K] -- btMultiBodyConstraintSolver::resolveConeFrictionConstraintRows, the
                             * path PyBullet takes unless setPhysicsEngineParameter(enableConeFriction=0) (the reference never calls it,
                             * simulation.py:13-35): both rows' unclamped sums against the same delta-velocities, the pair projected
                             * radially onto the disc of radius mu lambda_n.  DESIGN.md section 3 ([K] ledger) has the measured difference. */
  double kp, kd;            /* config 'gains' (configs/basic_pd.yaml:6) */
  double max_torque;        /* solo.py:53 max_joint_torque = 3 */
  double sim_dt;            /* solo.py:22 scene_timestep = 1/240 */
  double reward_dt;         /* stands in for the undefined scene.dt of baseEnv.py:137 (1/60) */
  double gravity;           /* simulation.py:19: 9.81 (pointing -z) */
  double erp;               /* contact/limit error-reduction (0.2, K7) */
  double linear_slop;       /* PyBullet solver linearSlop 1e-5 */
  double warmstart;         /* warm-start factor on cached normal impulses.  Default 0: btMultiBodyConstraintSolver starts every
                             * multibody contact row at zero impulse (its warm start is disabled in the source: "issues gaining
                             * energy") [K].  btContactSolverInfo's 0.85 (rigid bodies) was the default of rounds 1-2; with it the
                             * residual exit below destabilises a PD stance (measured) */
  double damping;           /* btMultiBody linear = angular damping 0.04 (K3) */
  double max_velocity;      /* generalized velocity clamp 100 (K5) */
  double joint_limit;       /* +-10 rad (URDF; solo.py:109) */
  double goal_radius;       /* solo.py:141 goal_radius = 2.0 */
  /* Treadmill (simulation.py:45-77): a static 50 x 2 zero heightfield = a 49 m x 1 m strip at z = 0 centred on
   * y = +-treadmill_offset (sign redrawn at every reset, simulation.py:72-74), Bullet default friction 0.5; its
   * velocity is set on a mass-0 body and has no effect.  Modelled as: a contact whose point lies on the strip
   * (|y - y_strip| <= treadmill_half_width) gets friction link_mu * treadmill_friction.  The feet sensor (solo.py:313-317
   * queries the plane body) still reports such a foot: the infinite plane lies under the strip as well. */
  double treadmill_offset;      /* 0.49 (simulation.py:49) */
  double treadmill_half_width;  /* 0.5: (numHeightfieldColumns - 1) / 2 grid units */
  double treadmill_friction;    /* 0.5: Bullet's default lateral friction of the heightfield body */
  /* PyBullet's solverResidualThreshold (1e-7, set by its physics server): the PGS loop of a sub-step
   * ends after the first iteration whose largest squared velocity-level change, max_rows (delta_impulse / jacDiagABInv)^2, is
   * <= this value (or after solver_iterations).  Default 1e-7 = the reference's setting (it never calls
   * setPhysicsEngineParameter, simulation.py:13-35).  0 = always run solver_iterations sweeps (the default of rounds 1-2).
   * Measured on the oracle: with warmstart = 0 the exit leaves a PD stance stable over 1000 control steps
   * at a mean of ~12 sweeps; with warmstart = 0.85 it does not -- the pair (0, 1e-7) is what Bullet's multibody solver runs [K]. */
  double solver_residual_threshold;
  /* Error reduction of the CONTACT rows (Bullet: btContactSolverInfo::m_erp2, read by setupMultiBodyContactConstraint); `erp` above is
   * m_erp, which the joint-limit rows use.  PyBullet's physics server sets m_erp2 = 0.08 beside m_erp = 0.2 [K]; rounds 1-3 used one
   * value (0.2) for both.  DESIGN.md section 3 ([K] ledger) has the measured difference. */
  double contact_erp;
  /* Collision margin around every collision shape [m].  Bullet gives the convex hulls of a URDF import a 1 mm margin (gUrdfDefaultCollisionMargin,
   * SURVEY.md Appendix B K6 [K]): the effective shape is the hull swept by a sphere of that radius, so every support point lies the
   * margin further down.  The analytic primitives were fitted to the bare meshes (tools/compile_model.py); rounds 1-3 ran them bare (0). */
  double collision_margin;
} solorl_config;

/* Struct-of-arrays info block (replaces the per-env dicts of baseEnv.py:62-66).  Every pointer is
 * a device array of num_envs elements, or NULL to skip that field. */
typedef struct solorl_info_soa {
  /* info['timeout'] (valid where done): 1 where the time limit ended the episode, and the time limit is tested first -- a fall on the
   * very last step is a timeout (baseEnv.py:164-167).  0 for an env the non-finite-state guard, a reached pointgoal or a
   * solorl_terminate rule ended.  The pointers are read per call: a caller that wants a step's flags in a row of its own (the
   * rollout rows solorl_compute_returns_tl reads) passes that step a block with this pointer set to the row. */
  uint8_t* timeout;
  uint8_t* success;          /* info['success'] (valid where done) */
  uint8_t* nan_reset;        /* env was force-reset because its state went non-finite */
  int32_t* episode_length;   /* info['episode_length'] = timestep */
  float*   episode_reward;   /* info['episode_reward'] = LAST step reward (baseEnv.py:65) */
  float*   goals_reached;    /* info['goals_reached'] */
  float*   dr_stand;         /* info['dr/stand_rew'] running sum */
  float*   dr_joint_pose;    /* info['dr/joint_pose_rew'] */
  float*   dr_torque;        /* info['dr/torque_rew'] */
  float*   dr_balance;       /* info['dr/roll_pitch_balance_rew'] */
  float*   dr_progress;      /* info['dr/progress_rew'] */
  /* Finished-episode accumulators, field-major [SOLORL_EPSTAT_FIELDS][num_envs], or NULL: at every env-step that ends
   * an episode the engine ADDS that episode's values to the env's own column (no atomics: deterministic); the caller
   * reduces over envs and zeroes the block whenever it logs.  Replaces iterating N info dicts per step
   * (agents/ppo/train.py:90-100).  Fields: 0 episodes finished, 1 sum info['episode_reward'], 2 sum
   * info['episode_length'], 3 sum info['success'], 4..8 sums of the info['dr/...'] terms (stand, joint_pose, torque, balance,
   * progress), 9 episodes ended by the non-finite-state guard (not counted in 0..8). */
  float*   ep_stats;
  /* [num_envs][act_dim], or NULL: the joint torques this step applied (solo.py:224-259 after the clip / the PD law of
   * controllers/PD.py:3-10) -- what the reference hands to p.setJointMotorControlArray(TORQUE_CONTROL, forces=...).  Lets a
   * test compare the engine's PD arithmetic with the reference's own PD() outputs (tests/golden/pd_golden.json). */
  float*   applied_torque;
} solorl_info_soa;
#define SOLORL_EPSTAT_FIELDS 10

/* Physical + bookkeeping state of ONE env in a fixed, precision-independent (double) layout;
 * used by solorl_get_state/solorl_set_state (HOST pointers) for parity tests, and as the row type of the batched
 * solorl_get_states / solorl_set_states (DEVICE rows). */
#define SOLORL_STATE_MAX_DOF 12
#define SOLORL_STATE_MAX_PRIMS 24
#define SOLORL_STATE_MAX_OBS 42
#define SOLORL_STATE_MAX_HISTORY 4
typedef struct solorl_env_state {
  double pos[3], quat[4] /* x y z w */, lin_vel[3], ang_vel[3];
  double q[SOLORL_STATE_MAX_DOF], qd[SOLORL_STATE_MAX_DOF], tau[SOLORL_STATE_MAX_DOF];
  double lambda_prev[SOLORL_STATE_MAX_PRIMS];  /* warm-start normal impulses per collision primitive */
  double hist[SOLORL_STATE_MAX_HISTORY][SOLORL_STATE_MAX_OBS];   /* state_history, [0] = newest */
  double goal[2], potential, progress, goals_reached, env_goals_reached;
  double dr[5];                                /* stand, joint_pose, torque, balance, progress */
  double treadmill_y;                          /* centre line of the treadmill strip (+-treadmill_offset; 0 if unused) */
  int32_t timestep, need_reset;
  int32_t contact_mask;  /* bit p (0..23): primitive p was in contact in the last sub-step; bit 24+f: foot f's contact
                          * point was on the treadmill strip (strip friction; the feet sensor reports it all the same) */
  int32_t rng_counter;
} solorl_env_state;

typedef struct solorl_env solorl_env;

/* Fills *cfg with the reference's defaults for (robot, task). */
int solorl_default_config(solorl_config* cfg, int robot, int task);

/* num_envs environments on HIP device `device_id`; `seed` + `env_id_offset` key the per-env
 * Philox streams (global env id = env_id_offset + i). */
int solorl_create(const solorl_config* cfg, int num_envs, int device_id, uint64_t seed,
                  int64_t env_id_offset, solorl_env** out);
int solorl_destroy(solorl_env* env);

int solorl_dims(const solorl_env* env, int* obs_dim, int* act_dim, int* num_envs);

int solorl_reset(solorl_env* env, float* obs_out /* [N*O] */, void* stream);
int solorl_step(solorl_env* env, const float* actions /* [N*A] */, float* obs_out /* [N*O] */,
                float* reward_out /* [N] */, uint8_t* done_out /* [N] */,
                const solorl_info_soa* info_out /* host struct of device pointers, or NULL */,
                void* stream);
int solorl_get_observation(solorl_env* env, float* obs_out, void* stream);
int solorl_increment_curriculum(solorl_env* env, double value);

/* Read-only properties of a handle (no reference counterpart): how this handle's batch is mapped and solved, so that a benchmark
 * or a scaling run can record and pin what it measured.  Names: "lanes_per_env" (16 team mode / 1 lane mode), "sweep_variant"
 * (2: PGS sweep with the K7 residual exit -- the default, one variant at every batch size; 1 / 0: fixed-iteration sweep,
 * software-pipelined / plain -- chosen by grid size when solver_residual_threshold = 0 unless SOLORL_PGS_PIPE pins it, the last bits
 * of an env then depend on which side of one wavefront per SIMD its batch is), "max_contacts", "max_limit_rows", "f64",
 * "sort" (1: contact-count sorting, SOLORL_SORT=1 at solorl_create with at least two envs: solorl_step ping-pongs two state buffers),
 * "step_n_one_launch" (1: solorl_step_n / solorl_rollout run K steps in one launch; 0: lane mode or contact-count sorting, where
 * solorl_step_n issues K ordinary steps and solorl_rollout is refused), "helper_wave" (1: solorl_step, solorl_step_act and a
 * one-step solorl_step_n launch two wavefronts per workgroup, the second one running the collision front of every sub-step beside the
 * first one's leg dynamics -- fp32 team mode without sorting while the batch gives every SIMD at most one workgroup, unless
 * SOLORL_HELPER_WAVE=0 pins it off; results are bitwise the same either way.  SOLORL_HELPER_WAVE=1 beyond that rule makes
 * solorl_create fail with SOLORL_ERR_INVALID).
 * Unknown name: SOLORL_ERR_INVALID. */
int solorl_get_property(const solorl_env* env, const char* name, double* value);

int solorl_get_state(solorl_env* env, int env_index, solorl_env_state* out /* host */);
int solorl_set_state(solorl_env* env, int env_index, const solorl_env_state* in /* host */);

/* Batched state access: the state of every env of the handle as `solorl_env_state rows[num_envs]` in DEVICE memory, moved by one kernel
 * launch on `stream`.  No host synchronisation, no allocation (capturable in a HIP graph, unlike solorl_get_state / solorl_set_state).
 *   Row i is ENV i of the handle (whatever storage slot the engine keeps it in; with contact-count sorting the kernel reads the
 *   slot -> env map itself).  mask: [num_envs] bytes on the device, or NULL = every env; a row whose mask byte is 0 is neither read
 *   nor written, in either direction.
 *   Values exactly as the per-env functions give and take them: an fp32 handle rounds each double to float on write and widens on
 *   read, an fp64 handle copies bits; `tau`, the joints 8..11 of a Solo8 handle and history levels the handle does not store read 0
 *   and are ignored on write.
 * solorl_set_states copies the member groups named by `fields` and leaves everything else of the env as it is:
 *   POSE pos, quat (and the engine's previous-xy, set to pos xy as solorl_set_state does) | VEL lin_vel, ang_vel | JOINT_POS q |
 *   JOINT_VEL qd | CONTACT lambda_prev, contact_mask | HISTORY hist | TASK goal, potential, progress, goals_reached,
 *   env_goals_reached, dr, treadmill_y | COUNTERS timestep, need_reset, rng_counter.
 *   NOTHING ELSE IS DERIVED on a partial write: a caller who moves a pointgoal env with POSE also writes `potential` (the distance to the
 *   goal the next step's `progress` is measured from) with TASK; one who changes q leaves the history's old angles unless it writes
 *   HISTORY -- or calls solorl_restart_history afterwards, which rebuilds the levels from the new state bit for bit.  fields == 0 or bits outside SOLORL_SF_ALL: SOLORL_ERR_INVALID.
 *   "Has been reset": solorl_set_states(mask = NULL, fields = SOLORL_SF_ALL) gives every env a complete state and marks the handle as
 *   reset, whatever the rows' need_reset members say -- the host cannot read them without synchronising, so they are the caller's
 *   business (solorl_set_state, which sees its one host row, marks the handle only when that row's need_reset is 0).  Any other
 *   solorl_set_states, and solorl_reset_masked, return SOLORL_ERR_STATE on a handle that has not been reset.  solorl_get_states is
 *   always allowed.
 * solorl_reset_masked: solorl_reset for the envs whose mask byte is non-zero -- the same snapshot draw from the env's own Philox counter
 *   that a full reset or an in-step auto-reset of that env would make next.  obs_out ([N*O], or NULL): rows of the selected envs only.
 * Null handle, out, in, or (solorl_reset_masked) mask: SOLORL_ERR_INVALID, the message names the function. */
enum { SOLORL_SF_POSE = 1, SOLORL_SF_VEL = 2, SOLORL_SF_JOINT_POS = 4, SOLORL_SF_JOINT_VEL = 8, SOLORL_SF_CONTACT = 16,
       SOLORL_SF_HISTORY = 32, SOLORL_SF_TASK = 64, SOLORL_SF_COUNTERS = 128, SOLORL_SF_ALL = 255 };
int solorl_get_states(solorl_env* env, const uint8_t* mask /* [N] device, or NULL = all */,
                      solorl_env_state* out /* [N] DEVICE rows */, void* stream);
int solorl_set_states(solorl_env* env, const uint8_t* mask, const solorl_env_state* in /* [N] DEVICE rows */,
                      uint32_t fields, void* stream);
int solorl_reset_masked(solorl_env* env, const uint8_t* mask /* [N] device, not NULL */,
                        float* obs_out /* [N*O] or NULL */, void* stream);

/* Random base kicks drawn and applied on the device (no reference counterpart; what domain-randomised training calls "pushes").  A kick
 * is a change of the base's world-frame velocity, as SoloVecEnv.push() makes one through solorl_get_states / solorl_set_states; here
 * every env receives kicks at random intervals from a Philox stream of its own, by ONE launch per control step that touches six state
 * words of the kicked envs and nothing of the others.  The step kernels know nothing of it: a caller issues solorl_perturb between two
 * steps (SoloVecEnv does, right before each step launch, once a perturbation is set).
 * solorl_set_perturbation: allocates (first call) and initialises two per-env arrays owned by the handle and indexed by ENV id -- the
 *   countdown to the env's next kick and the number of kicks it has drawn -- and latches *p; calling it again restarts the schedule
 *   from block 0; p == NULL switches the perturbation off and frees the arrays (solorl_destroy frees them too).  Synchronises the host,
 *   as solorl_create does: not capturable.  SOLORL_ERR_INVALID for an interval outside 1 <= min <= max or a negative or non-finite
 *   amplitude (the handle's perturbation stays as it was).
 * solorl_perturb: one launch on `stream`, no allocation, no host synchronisation (capturable).  Per env: countdown -= 1; at 0 the env draws
 *   kick j (j = its kick count), applies it, counts it and draws its next countdown.  kick_out ([N][6]: lin x y z, ang x y z; or NULL)
 *   receives the kick applied by THIS call, zeros for an env that was not kicked.  An env that is not kicked has no state word written;
 *   of a kicked env only the components with a non-zero amplitude are (v + 0.0 would turn -0.0 into +0.0): a zero amplitude is an exact
 *   no-op and its kick_out entry is +0.0.  SOLORL_ERR_STATE before solorl_set_perturbation or before the handle's first reset.
 * solorl_get_perturbation: copies the two arrays out in one launch (either pointer may be NULL, not both).
 * Draws (all of them a function of seed, global env id, the call count and *p -- never of the state or the actions):
 *   key      the handle's seed (lo, hi), as for the env's own stream
 *   counter  (gid_lo, gid_hi, block, 4) with gid = env_id_offset + i.  The env's own stream uses 1, 2 and 3 in the last word with
 *            rng_counter in the third; a kick never reads or advances rng_counter.
 *   block 0          word 0 -> the first countdown
 *   block 1 + 2 j    words 0, 1, 2 -> kick j's lin x, y, z; word 3 -> the countdown to kick j + 1
 *   block 2 + 2 j    words 0, 1, 2 -> kick j's ang x, y, z
 *   uniform    u = (word >> 8) * 2^-24; component = (2 u - 1) * max, in double (2 u - 1 is exact: one rounding)
 *   countdown  interval_min + word % (interval_max - interval_min + 1)
 *   addition   v <- T(double(v) + kick), T the engine's arithmetic type: one rounding, bitwise what push() gives for the same kick as a
 *              float64 tensor on fp32 and fp64 handles alike
 *   schedule   counts solorl_perturb calls and ignores episode boundaries: auto-resets and solorl_reset_masked leave it alone
 *   shards     keyed by global env id: W handles of N envs at offsets k N kick like one handle of W N envs */
typedef struct solorl_perturbation {
  int32_t interval_min, interval_max;   /* control steps between two kicks of an env, uniform in [min, max]; 1 <= min <= max */
  double  max_lin_vel[3];               /* a kick adds U(-m, m) to lin_vel[i]; 0 = that component is never touched */
  double  max_ang_vel[3];               /* the same for ang_vel[i] */
} solorl_perturbation;
int solorl_set_perturbation(solorl_env* env, const solorl_perturbation* p /* host; NULL = switch off */);
int solorl_perturb(solorl_env* env, double* kick_out /* [N][6] device, or NULL */, void* stream);
int solorl_get_perturbation(solorl_env* env, int32_t* countdown_out /* [N] device */, uint32_t* kicks_out /* [N] device */, void* stream);

/* Derived quantities of a batch of state rows: link poses and velocities, the collision primitives' support points with their
 * velocities and normal forces, centre of mass, energy and momentum -- what the reference reads from PyBullet (getLinkState,
 * getContactPoints, the BodyPart poses of pybullet_envs.robot_bases) and Isaac-style vec-envs expose as rigid_body_state /
 * net_contact_force tensors.  One kernel launch on `stream`, one row out per row in.
 *   Links in the order of the model table, solorl_model_data: link 0 = the base (a foot is a fixed child of its lower leg); primitives likewise
 *   (0..11 base points, 12 + 2 leg knee, 13 + 2 leg foot, 20 + leg shoulder housing of a Solo12).  Links 13..16 and primitives
 *   20..23 of a Solo8 read 0.
 *   prim_point is the support point of the BARE shape -- the engine's own formulas (disc_point, ring_disc_point, the base points of the
 *   model table), what the oracle's oracle_prim_points returns; the contact test of a sub-step compares its z - collision_margin with the
 *   primitive's margin.  Arithmetic is fp64 whatever the precision of the engine that produced the rows: an fp32 engine's collision front
 *   sees the same points up to float rounding.
 *   prim_force: the normal force of the LAST sub-step of the last step, lambda_prev[p] / sim_dt where contact_mask bit p is set, else 0.
 *   Energy and momentum as the oracle's oracle_energy_momentum: link inertia per use_urdf_inertia (0: Bullet's box rule, 1: the URDF
 *   tensor), potential = sum m g c_z, angular momentum about the WORLD origin.
 * A function of the rows and of cfg's robot, use_urdf_inertia, sim_dt and gravity only (no handle; rows from any source).  mask: [n] bytes on
 * the device or NULL = every row; a row whose mask byte is 0 is neither read nor written.  `out` must not overlap `states`.  No host
 * synchronisation, no allocation: capturable.  Non-finite members of a row give non-finite members of that row's output and nothing
 * else (no index is computed from data).
 * Null cfg, states or out, n < 1, a robot that is neither SOLORL_ROBOT_*, sim_dt <= 0 or a non-finite sim_dt / gravity: SOLORL_ERR_INVALID,
 * the message names the function (checked before any HIP call). */
#define SOLORL_KIN_MAX_LINKS 17
typedef struct solorl_env_kin {
  double link_pos[SOLORL_KIN_MAX_LINKS][3];      /* world position of each link frame's origin */
  double link_quat[SOLORL_KIN_MAX_LINKS][4];     /* x y z w, link axes -> world, unit, w >= 0 */
  double link_com[SOLORL_KIN_MAX_LINKS][3];      /* world position of the link's centre of mass */
  double link_com_vel[SOLORL_KIN_MAX_LINKS][3];  /* world velocity of that point */
  double link_ang_vel[SOLORL_KIN_MAX_LINKS][3];  /* world angular velocity of the link */
  double prim_point[SOLORL_STATE_MAX_PRIMS][3];  /* support point of each collision primitive (bare shape, see above) */
  double prim_vel[SOLORL_STATE_MAX_PRIMS][3];    /* velocity of the link's material point at prim_point */
  double prim_force[SOLORL_STATE_MAX_PRIMS];     /* normal force [N] of the last sub-step */
  double com[3], com_vel[3], mass;
  double kinetic, potential, lin_mom[3], ang_mom[3];
} solorl_env_kin;
int solorl_kinematics(const solorl_config* cfg, const solorl_env_state* states /* [n] DEVICE rows */,
                      const uint8_t* mask /* [n] device, or NULL = all */, int n,
                      solorl_env_kin* out /* [n] DEVICE rows */, int device_id, void* stream);

/* Rigid-body dynamics tensors of a batch of state rows: the joint-space mass matrix, the bias and gravity forces, and per foot the
 * Jacobian, its Jdot v and the point it belongs to -- the members of the rigid_body_state / net_contact_force family that
 * solorl_kinematics leaves out (Isaac-style jacobian and mass_matrix tensors).  One kernel launch on `stream`, one row out per row in.
 *   Generalised velocity v = [lin_vel(3), ang_vel(3), qd[0..11]]: the state row's own members in the row's own order; lin_vel is the
 *   world velocity of the base frame's origin `pos`, ang_vel the world angular velocity.  Dual forces are [world force on the base, world
 *   torque about pos, joint torques].  A Solo8 has 14 coordinates: rows and columns 14..17 of every member read exactly 0.  The oracle
 *   (oracle_mass_matrix) orders [angular, linear, joints]: the same quantities under the permutation that swaps the first two triples.
 *   mass_matrix: M(q), kinetic = 1/2 v^T M v.  Link inertia per use_urdf_inertia (0: Bullet's box rule, 1: the URDF tensor); a foot is
 *   counted with its lower leg.  Symmetric to the bit.  A leg's joints couple with the base and with the same leg only: the blocks
 *   between different legs read exactly +0.0.
 *   bias: h(q, v) of  M udot + bias = tau + J^T f : gravity, Coriolis and centrifugal terms, the gyroscopic term w x I w and Bullet's
 *   link damping K3 (F = -m v_c (k + k |v_c|), T = -I w (k + k |w|), k = cfg->damping) -- what oracle_mass_matrix returns as h and what
 *   the engine's unconstrained sub-step integrates.  For the rigid-body terms alone pass a config copy with damping = 0.
 *   gravity: bias at v = 0.  Entries 0..2 are (0, 0, total mass x g), 3..5 the moment of the weight about pos, the joint entries
 *   dV/dq_j of solorl_env_kin.potential: tau = gravity[6..] is the gravity-compensation torque, the one that holds the joints against the
 *   links' weight (udot = 0 at rest in the equation above; -gravity[6..] is the generalised force the weight exerts).
 *   foot_pos[L]: the support point of the foot primitive 13 + 2 L of leg L (FL, FR, HL, HR), = solorl_env_kin.prim_point[13 + 2 L].
 *   foot_jac[L]: the 3 x 18 Jacobian of the lower leg's MATERIAL point at foot_pos[L]: foot_jac[L] v = solorl_env_kin.prim_vel[13 + 2 L],
 *   foot_jac[L]^T f = the generalised force of a world force f at the foot.  Columns of the other legs' joints read 0.
 *   foot_acc_bias[L]: Jdot v, the acceleration of that material point when all generalised accelerations are zero.
 * A function of the rows and of cfg's robot, use_urdf_inertia, gravity and damping only (no handle; rows from any source); fp64 whatever
 * the precision of the engine that produced the rows.  mask: [n] bytes on the device or NULL = every row; a row whose mask byte is 0 is
 * neither read nor written.  `out` must not overlap `states`.  No host synchronisation, no allocation: capturable.  Non-finite members
 * of a row give non-finite members of that row's output and nothing else (no index is computed from data).
 * Null cfg, states or out, n < 1, a robot that is neither SOLORL_ROBOT_*, a non-finite gravity, a non-finite or negative damping:
 * SOLORL_ERR_INVALID, the message names the function (checked before any HIP call). */
#define SOLORL_DYN_NV 18
typedef struct solorl_env_dyn {
  double mass_matrix[SOLORL_DYN_NV][SOLORL_DYN_NV];
  double bias[SOLORL_DYN_NV];
  double gravity[SOLORL_DYN_NV];
  double foot_jac[4][3][SOLORL_DYN_NV];
  double foot_acc_bias[4][3];
  double foot_pos[4][3];
} solorl_env_dyn;                     /* 600 doubles = 4800 B */
int solorl_dynamics(const solorl_config* cfg, const solorl_env_state* states /* [n] DEVICE rows */,
                    const uint8_t* mask /* [n] device, or NULL = all */, int n,
                    solorl_env_dyn* out /* [n] DEVICE rows */, int device_id, void* stream);

/* Shaped reward terms of a batch of state rows: the foot, smoothness and energy terms that legged-RL tasks add to a task reward (Isaac-style
 * legged_gym reward functions; no reference counterpart: the reference pays stand, joint pose, torque, balance and progress only).  A third
 * row query beside solorl_kinematics and solorl_dynamics: a pure function of its arguments, no handle; ONE kernel launch on `stream`, no
 * allocation, no host synchronisation (capturable).  A caller issues it after a step, on the state AFTER that step (solorl_get_states), with
 * the actions, the done flags and the reward of that step; the terms that need the previous step (joint acceleration, action rate, feet air
 * time) keep it in `mem`, one caller-owned device row per env that this call reads and rewrites.
 * Notation: R0 = the rotation matrix of the row's quaternion as it is (what solorl_kinematics uses); v_b = R0^T lin_vel, w_b = R0^T ang_vel,
 * g_b = R0^T (0, 0, -1); j runs over the robot's 8 or 12 joints; dtc = sim_dt * frame_skip; for foot f = FL, FR, HL, HR: p_f, u_f, F_f are
 * solorl_env_kin's prim_point, prim_vel and prim_force of the foot primitive 13 + 2 f (the same functions compute them), c_f that
 * primitive's contact_mask bit; a = this call's action row (raw, unclipped).
 *    k  name               value
 *    0  lin_vel_z          v_b.z^2
 *    1  ang_vel_xy         w_b.x^2 + w_b.y^2
 *    2  orientation        g_b.x^2 + g_b.y^2
 *    3  base_height        (pos.z - base_height_target)^2
 *    4  torques            sum_j tau_j^2                    (the row's tau)
 *    5  joint_vel          sum_j qd_j^2
 *    6  joint_acc          valid ? sum_j ((qd_j - prev_qd_j) / dtc)^2 : 0
 *    7  action_rate        valid ? sum_j (a_j - prev_action_j)^2 : 0
 *    8  power              sum_j |tau_j qd_j|
 *    9  foot_slip          sum_f c_f (u_f.x^2 + u_f.y^2)
 *   10  foot_clearance     sum_f (1 - c_f) (p_f.z - foot_clearance_target)^2 sqrt(u_f.x^2 + u_f.y^2)
 *   11  foot_force         sum_f max(0, F_f - foot_force_max)
 *   12  feet_air_time      sum_f first_f (air_f - air_time_target)
 *   13  collision          number of set contact_mask bits among the robot's primitives other than the four foot primitives
 *   14  tracking_lin_vel   exp(-((v_b.x - cmd_lin_vel[0])^2 + (v_b.y - cmd_lin_vel[1])^2) / tracking_sigma)
 *   15  tracking_yaw_rate  exp(-(w_b.z - cmd_yaw_rate)^2 / tracking_sigma)
 *   Term 12, in order: air_f = air_time[f] + dtc; first_f = valid && c_f && !(prev_contact bit f); the term reads air_f; afterwards
 *   air_time[f] = c_f ? 0 : air_f.  All arithmetic is fp64, sums in index order.  No scaling by dt is applied: the weights carry it.
 * A live row with done == 0: terms_out[i][k] = the raw value of every term, whatever the weights; s = sum_k weight[k] term_k in index
 *   order; reward[i] = (float)((double)reward[i] + s), rounded once; ep_sum[k] += weight[k] term_k; prev_action = a, prev_qd = qd,
 *   prev_contact = (c_f), valid = 1.
 * A live row with done != 0 (the row holds the post-reset state and the terminal reward is the reference's override): reward[i] is
 *   untouched, terms_out[i][:] = 0; ep_out[0][i] += 1 and ep_out[1 + k][i] += ep_sum[k] (the contract of ep_stats: the caller reduces
 *   and zeroes); ep_sum, air_time, prev_contact and valid are zeroed (prev_action and prev_qd are not read while valid is 0).
 * A masked row (mask byte 0): nothing of it is read or written, in any array.
 * Null cfg, p, states, actions or mem, n < 1, a robot that is neither SOLORL_ROBOT_*, a non-finite weight or parameter,
 * tracking_sigma <= 0, sim_dt <= 0 (or non-finite), frame_skip < 1: SOLORL_ERR_INVALID, the message starts with
 * "solorl_shape_reward:" (checked before any HIP call). */
#define SOLORL_SHAPE_TERMS 16
typedef struct solorl_shape_params {
  double weight[SOLORL_SHAPE_TERMS];           /* 0 = term off */
  double base_height_target, foot_clearance_target, foot_force_max, air_time_target;
  double cmd_lin_vel[2], cmd_yaw_rate, tracking_sigma;   /* base frame; sigma > 0 */
} solorl_shape_params;
typedef struct solorl_env_shape {              /* per-env memory, caller-owned DEVICE rows, 45 words = 360 B */
  double prev_action[12], prev_qd[12], air_time[4], ep_sum[SOLORL_SHAPE_TERMS];
  int32_t prev_contact /* bit f: foot f touched at the previous call */, valid /* 0: no previous step in this episode */;
} solorl_env_shape;
int solorl_shape_reward(const solorl_config* cfg, const solorl_shape_params* p,
                        const solorl_env_state* states /* [n] DEVICE rows, the state AFTER the step */,
                        const uint8_t* mask /* [n] or NULL */, int n,
                        const float* actions /* [n][act_dim], the raw actions of that step */,
                        const uint8_t* done /* [n] or NULL = none */,
                        solorl_env_shape* mem /* [n], in/out */, float* reward /* [n] in/out, or NULL */,
                        double* terms_out /* [n][16] raw term values, or NULL */,
                        double* ep_out /* [17][n] field-major, or NULL */, int device_id, void* stream);

/* Observation noise and actuation (no reference counterpart; the "sensor noise", "action latency" and "motor strength" randomisations of
 * sim-to-real training).  Both calls are handle-free: they work on the two arrays that cross the boundary between policy and engine and
 * on caller-owned DEVICE memory, know nothing of the step kernels, and are ONE launch on `stream` each, without allocation or host
 * synchronisation (capturable).  Everything is a function of seed, global env id gid = env_id_offset + i and a per-env count, so W
 * shards at offsets k n draw what one batch of W n rows draws.  Key of both streams: (seed_lo, seed_hi), as for the env's own stream.
 *
 * solorl_obs_noise: obs_out[i][c] = obs_in[i][c] + U(-scale[c], scale[c]) for every row whose mask byte is not 0 (mask == NULL: all).
 *   counter   (gid_lo, gid_hi, block, 5).  The env's own stream uses 1, 2 and 3 in the last word and the kicks use 4; a draw never
 *             reads or advances rng_counter.
 *   block     count[i] * B + b (mod 2^32) with B = ceil(D / 4); word w of block b belongs to component c = 4 b + w, words past D are unused
 *   uniform   u = (word >> 8) * 2^-24; e = (2 u - 1) * (double)scale[c]: the subtraction is exact, the product rounds once, in double
 *   output    obs_out[i][c] = (float)((double)obs_in[i][c] + e): one double addition, one rounding to float (no fused multiply-add)
 *   zero      scale[c] == 0 copies the input's bits (NaN payloads and -0.0 survive); in place such a component is left as it is
 *   live row  afterwards count[i] += 1
 *   masked    nothing of the row is read or written and count[i] does not advance
 *   The additive noise does not re-wrap a wrapped quantity (the Euler angles of the observation).  Rows whose D is a multiple of 4 in
 *   16-byte aligned arrays move as 16-byte words, every other shape word by word; the values are the same.
 *   Null scale, count, obs_in or obs_out, n < 1, D < 1 or D > 210 (42 words x 5 levels): SOLORL_ERR_INVALID, the message starts with
 *   "solorl_obs_noise:" (checked before any HIP call).
 *
 * solorl_actuate: actions_out[i] = the action the motors of env i receive for the raw action actions_in[i] -- delayed by the env's
 *   latency (drawn per episode, in control steps) and scaled by its per-joint gains (drawn per episode).  Per env, in this order:
 *   1 restart   r = (restart && restart[i]) || mem.episodes == 0: a zeroed row draws at its first call
 *   2 on r      e = mem.episodes; counter (gid_lo, gid_hi, 4 e, 6) word 0 -> latency = delay_min + word % (delay_max - delay_min + 1);
 *               counters (.., 4 e + 1 + j / 4, 6) word j % 4 -> gain[j] = (float)(1.0 + (2 u - 1) * gain_range), u as above: the product
 *               is rounded, then the sum, then the result goes to float (exactly 1.0f for gain_range == 0); fill = 0, episodes = e + 1
 *   3 delayed   d_j = (latency == 0 || fill == 0) ? in_j : buf[min(latency, fill) - 1][j]: until `latency` actions have arrived the
 *               episode's FIRST action is held (safe for torque and PD actions alike; never a zero or a stale action of the last episode)
 *   4 output    out_j = gain_range == 0 ? d_j (its bits) : (float)((double)gain[j] * (double)d_j)
 *   5 buffer    levels 0 .. delay_max - 2 move up by one, buf[0] = in, fill = min(fill + 1, delay_max); with delay_max == 0 nothing moves
 *               and fill stays 0.  Levels >= delay_max and joints >= act_dim are never read or written.
 *   actions_out may be actions_in.  Null p, mem, actions_in or actions_out, n < 1, act_dim not 8 or 12, a delay range outside
 *   0 <= delay_min <= delay_max <= SOLORL_DELAY_MAX, a gain_range that is not finite or outside [0, 1): SOLORL_ERR_INVALID, the message
 *   starts with "solorl_actuate:" (checked before any HIP call). */
int solorl_obs_noise(uint64_t seed, int64_t env_id_offset,
                     const float* scale   /* [D] device: half-width per observation component; 0 = component untouched */,
                     const uint8_t* mask  /* [n] device or NULL */, int n, int D,
                     uint32_t* count      /* [n] device, in/out: noise calls this env has received */,
                     const float* obs_in  /* [n][D] */, float* obs_out /* [n][D]; may be obs_in */,
                     int device_id, void* stream);
#define SOLORL_DELAY_MAX 4
typedef struct solorl_actuation {
  uint64_t seed; int64_t env_id_offset;
  int32_t act_dim /* 8 or 12 */, delay_min, delay_max /* 0 <= min <= max <= SOLORL_DELAY_MAX, control steps */, reserved;
  double gain_range;   /* per joint and episode: gain = 1 + U(-r, r); 0 <= r < 1; 0 = gains are exactly 1 and nothing is multiplied */
} solorl_actuation;
typedef struct solorl_env_actuator {      /* caller-owned DEVICE rows, 64 words = 256 B */
  float buf[SOLORL_DELAY_MAX][12];        /* buf[k] = the raw action received k + 1 calls ago in this episode */
  float gain[12];
  int32_t latency, fill /* raw actions buffered this episode, saturating at delay_max */;
  uint32_t episodes /* episodes drawn so far */; int32_t reserved;
} solorl_env_actuator;
int solorl_actuate(const solorl_actuation* p, int n, const uint8_t* restart /* [n] device or NULL */,
                   solorl_env_actuator* mem /* [n] in/out */, const float* actions_in /* [n][A] */,
                   float* actions_out /* [n][A]; may be actions_in */, int device_id, void* stream);

/* Velocity commands (no reference counterpart; the per-env commands of legged_gym-style tasks): every env holds a command (vx, vy in
 * m/s and a yaw rate in rad/s, base frame) drawn from ranges and drawn anew after a per-env number of control steps; the policy sees it
 * as three more observation words and the tracking terms of solorl_shape_reward_cmd compare the env against it.  Handle-free like the
 * two calls above: ONE launch on `stream`, no allocation, no host synchronisation (capturable); everything is a function of seed,
 * global env id gid = env_id_offset + i and the env's memory row, so W shards at offsets k n draw what one batch of W n rows draws.
 * Key (seed_lo, seed_hi).  Per live env, in this order:
 *   1 decide    the env draws now if (restart && restart[i]) || mem.draws == 0 (a zeroed row draws at its first call); otherwise
 *               countdown -= 1 and the env draws now if countdown == 0
 *   2 draw      d = mem.draws; counter (gid_lo, gid_hi, 2 d, 7) -- the env's own stream uses 1, 2, 3 in the last word, the kicks 4, the
 *               noise 5, the actuator draws 6; a draw never reads or advances rng_counter.
 *               word 0   interval = interval_min + word % (interval_max - interval_min + 1)
 *               word 1+k u_k = (word >> 8) * 2^-24; cmd_k = lo_k + u_k * (hi_k - lo_k): fp64, the difference, the product and the sum each
 *                        rounded (no fused multiply-add), so lo_k == hi_k gives exactly lo_k
 *               counter (gid_lo, gid_hi, 2 d + 1, 7) word 0: u < zero_prob sets all three components to 0 (stand still)
 *               then cmd_0 * cmd_0 + cmd_1 * cmd_1 < min_lin_norm * min_lin_norm sets cmd_0 = cmd_1 = 0 (each product rounded, then the sum)
 *               finally draws = d + 1 (mod 2^32) and countdown = interval
 *   3 output    cmd_out[i][k] = cmd_k; obs_out[i][0..D) = the bits of obs_in[i][0..D) (NaN payloads and -0.0 survive);
 *               obs_out[i][D + k] = (float)(cmd_k * obs_scale[k]), the product rounded in double first.  obs_in and obs_out may both be
 *               NULL: then only mem and cmd_out are written.  obs_in must not overlap obs_out (the row strides differ).
 *   masked      (mask byte 0) nothing of the row is read or written, in any array
 *   An obs_in that is 16-byte aligned is read as 16-byte words, any other word by word; obs_out is written word by word; the values
 *   are the same.  A heading command (a yaw rate derived from a target heading) is not offered: see DESIGN.md.
 *   Null p or mem, exactly one of obs_in and obs_out null, n < 1, obs_dim < 1 or > 210, a range that is not finite or has lo > hi, an
 *   obs_scale that is not finite, zero_prob outside [0, 1] (or NaN), min_lin_norm negative or not finite, an interval range outside
 *   1 <= interval_min <= interval_max <= 1 << 20: SOLORL_ERR_INVALID, the message starts with "solorl_commands:" (checked before any
 *   HIP call).
 *
 * solorl_shape_reward_cmd: solorl_shape_reward with the commands per env.  cmd != NULL: terms 14 and 15 of row i use cmd[i].cmd[0..2] in
 *   place of p->cmd_lin_vel[0..1] and p->cmd_yaw_rate (only the cmd member is read, of live rows only).  cmd == NULL: solorl_shape_reward,
 *   which is this call with NULL.  Its refusals carry the prefix "solorl_shape_reward:". */
typedef struct solorl_command_params {
  uint64_t seed; int64_t env_id_offset;
  double lo[3], hi[3];        /* vx, vy [m/s, base frame], yaw rate [rad/s]; finite, lo <= hi */
  double obs_scale[3];        /* the observation word is (float)(cmd_k * obs_scale[k]); finite */
  double zero_prob;           /* in [0, 1]: probability that a draw is the zero command (stand still) */
  double min_lin_norm;        /* >= 0: a drawn (vx, vy) shorter than this becomes (0, 0) */
  int32_t interval_min, interval_max;   /* control steps between draws, 1 <= min <= max <= 1 << 20 */
  int32_t obs_dim;            /* D: width of the engine's observation rows; 1 <= D <= 210 */
  int32_t reserved;
} solorl_command_params;
typedef struct solorl_env_command {     /* caller-owned DEVICE rows, 32 B */
  double cmd[3]; int32_t countdown; uint32_t draws;
} solorl_env_command;
int solorl_commands(const solorl_command_params* p, const uint8_t* mask /* [n] or NULL */,
                    const uint8_t* restart /* [n] or NULL */, int n, solorl_env_command* mem /* [n] in/out */,
                    const float* obs_in /* [n][D] or NULL */, float* obs_out /* [n][D+3] or NULL */,
                    double* cmd_out /* [n][3] or NULL */, int device_id, void* stream);
int solorl_shape_reward_cmd(const solorl_config* cfg, const solorl_shape_params* p,
                            const solorl_env_state* states, const uint8_t* mask, int n, const float* actions,
                            const uint8_t* done, solorl_env_shape* mem, float* reward, double* terms_out,
                            double* ep_out, const solorl_env_command* cmd /* [n] rows or NULL */,
                            int device_id, void* stream);

/* Early termination (no reference counterpart; the "base contact", "orientation" and "dof limit" terminations of legged_gym-style tasks).
 * The engine ends an episode at the time limit, at a reached goal and at pos.z < 0.05; a robot on its knees, on its side or on its back
 * stays alive.  A fourth handle-free row query beside solorl_kinematics, solorl_dynamics and solorl_shape_reward: a pure function of its
 * arguments, ONE kernel launch on `stream`, no allocation, no host synchronisation (capturable).  A caller issues it after a step, on the
 * state AFTER that step (solorl_get_states), with the done flags, the reward and the info block of that step, and then hands fired_out to
 * solorl_reset_masked as its mask:   step -> solorl_get_states -> solorl_terminate -> solorl_reset_masked(fired_out, obs rows).
 * The step kernels know nothing of it.
 * Rules (all arithmetic fp64, every product and sum rounded on its own, no fused multiply-add: every flag is specified to the bit; a
 * rule fires only on a FINITE tested value, so NaN and +-Inf members fire nothing -- non-finite states belong to the engine's own guard):
 *   HEIGHT   z = pos[2]:  z finite and z < min_height
 *   TILT     up_z = 1 - 2 (qx qx + qy qy) on the quaternion as it is in the row (the z component of the base's z axis, = cos of its
 *            angle to world z for a unit quaternion):  up_z finite and up_z < min_up_z
 *   CONTACT  some primitive p of contact_prims that the robot has (0..19 Solo8, 0..23 Solo12) has its contact_mask bit set and
 *            f = lambda_prev[p] / sim_dt (solorl_env_kin.prim_force) finite and f >= contact_force_min
 *   JOINT    some joint j < act_dim has q[j] finite and (q[j] < joint_lo[j] or q[j] > joint_hi[j])
 *   No rule fires on a row whose timestep < min_steps.
 * Rows:
 *   live, done[i] != 0 on entry     the engine ended and reset it, the row holds the new episode: fired_out[i] = 0, nothing else is written
 *   live, done[i] == 0, none fires  fired_out[i] = 0, nothing else is written
 *   live, done[i] == 0, some fire   fired_out[i] = all the bits that fire; done[i] = 1; reward[i] = (float)terminal_reward (an override,
 *                                   as the engine's own -10 is); the info and term_stats writes below
 *   masked (mask byte 0)            nothing of the row is read or written, in any array (a caller that uses fired_out as a mask zeroes
 *                                   it first)
 * Info writes of a row where a rule fires, what the engine writes when its own fall rule ends an episode (each member may be NULL):
 *   timeout[i] = 0, success[i] = 0, episode_reward[i] = reward[i];  the ep_stats column: [0] += 1, [1] += reward, [2] += (float)timestep,
 *   [3] += 0, [4 + k] += (float)dr[k];  the other info fields already hold this step's values.
 *   term_stats ([1 + SOLORL_TERM_RULES][n] floats, field-major, or NULL): [0][i] += 1 and [1 + k][i] += 1 for every rule bit k that fired
 *   -- the contract of ep_stats: one column per env, no atomics, the caller reduces and zeroes.
 * A function of the rows, *p and cfg's robot and sim_dt only.
 * Null cfg, p, states, done, reward or fired_out, n < 1, a robot that is neither SOLORL_ROBOT_*, sim_dt <= 0 (or non-finite), rules == 0 or
 * bits outside the four, min_steps < 0, a non-finite threshold of an enabled rule (joint limits: of the joints j < act_dim),
 * contact_force_min < 0, joint_lo[j] > joint_hi[j] for a j < act_dim, a non-finite terminal_reward, contact_prims naming primitives the
 * robot does not have while CONTACT is enabled: SOLORL_ERR_INVALID, the message starts with "solorl_terminate:" (checked before any HIP
 * call). */
#define SOLORL_TERM_RULES 4
enum { SOLORL_TERM_HEIGHT = 1, SOLORL_TERM_TILT = 2, SOLORL_TERM_CONTACT = 4, SOLORL_TERM_JOINT = 8 };
typedef struct solorl_termination {
  uint32_t rules;            /* bit set of the enabled rules; 0 is refused */
  int32_t  min_steps;        /* >= 0: no rule fires on a row whose timestep < min_steps */
  uint32_t contact_prims;    /* bit p (0..23): primitive p counts for the contact rule */
  int32_t  reserved;
  double   min_height;       /* HEIGHT:  pos.z < min_height */
  double   min_up_z;         /* TILT:    up_z < min_up_z (cos of the largest allowed angle between the base's z axis and world z) */
  double   contact_force_min;/* CONTACT: some p in contact_prims has its contact_mask bit set and lambda_prev[p] / sim_dt >= contact_force_min (>= 0) */
  double   joint_lo[12], joint_hi[12];   /* JOINT: some j < act_dim has q[j] < joint_lo[j] or q[j] > joint_hi[j] */
  double   terminal_reward;  /* the reward a terminated row receives (an override, as the engine's own -10 is) */
} solorl_termination;
int solorl_terminate(const solorl_config* cfg, const solorl_termination* p,
                     const solorl_env_state* states /* [n] DEVICE rows, the state AFTER the step */,
                     const uint8_t* mask /* [n] or NULL */, int n,
                     uint8_t* done /* [n] in/out */, float* reward /* [n] in/out */,
                     uint8_t* fired_out /* [n]: the rule bits that fired, 0 where none */,
                     const solorl_info_soa* info /* or NULL; arrays of n elements, ep_stats [FIELDS][n] */,
                     float* term_stats /* [1 + SOLORL_TERM_RULES][n] or NULL */, int device_id, void* stream);

/* Randomised initial states (no reference counterpart; the "initial state distribution" of domain-randomised legged-robot training).  A
 * reset copies one of 7 snapshots (14 with the treadmill): every episode starts at rest, facing +x, with the same joint angles.  A fifth
 * handle-free row query beside solorl_kinematics, solorl_dynamics, solorl_shape_reward and solorl_terminate: a pure function of its
 * arguments, ONE kernel launch on `stream`, no allocation, no host synchronisation (capturable).  It changes state ROWS in place; a
 * caller moves them in and out of a handle with solorl_get_states / solorl_set_states and then restarts the handle's history:
 *   solorl_get_states(mask, rows) -> solorl_randomize_reset(rows, mask, count) ->
 *   solorl_set_states(mask, rows, POSE | VEL | JOINT_POS | JOINT_VEL | CONTACT) -> solorl_restart_history(mask, obs rows).
 * The step kernels know nothing of it.
 * Draws (all of them a function of seed, global env id, the env's episode index and *p -- never of the state or the actions; all
 * arithmetic fp64, every product and sum rounded on its own, no fused multiply-add):
 *   episode    k = count[i] on entry; count[i] = k + 1 on return, for every selected row.  Valid for k < 2^28 (16 k + b is a 32-bit word).
 *   key        the seed (lo, hi), as for the env's own stream
 *   counter    (gid_lo, gid_hi, 16 k + b, 8) with gid = env_id_offset + i.  The env's own stream uses 1, 2 and 3 in the last word, the
 *              kicks 4, the noise 5, the actuator draws 6, the commands 7; none of these draws reads or advances rng_counter.
 *   block b = 0, 1, 2    words 0..3 -> q[4 b .. 4 b + 3], half-widths joint_pos[..]
 *   block b = 3, 4, 5    words 0..3 -> qd[4 (b - 3) .. 4 (b - 3) + 3], half-widths joint_vel[..]
 *   block b = 6          words 0, 1, 2 -> lin_vel x, y, z, half-widths lin_vel[..]; word 3 -> the yaw angle psi, half-width yaw
 *   block b = 7          words 0, 1, 2 -> ang_vel x, y, z, half-widths ang_vel[..]; word 3 -> the roll angle phi, half-width roll
 *   block b = 8          word 0 -> the pitch angle theta, half-width pitch
 *   A Solo8 draws nothing for joints 8..11 (blocks 2 and 5) and leaves those words of the row alone.
 *   uniform    u = (word >> 8) * 2^-24;  d = (2 u - 1) * a in double (2 u - 1 is exact: one rounding);  member <- member + d
 *   zero       a half-width of 0 is an exact no-op: the word is not written, -0.0 survives (the convention of solorl_perturb)
 *   q          q[j] <- fmin(fmax(q[j] + d, -joint_limit), +joint_limit) with cfg's joint_limit, where joint_pos[j] != 0 (C's fmax / fmin:
 *              a q[j] that is NaN on entry comes out as -joint_limit)
 * Orientation, unless yaw, roll and pitch are all 0 (then quat is not touched, not even normalised):
 *   quat <- Rz(psi) * quat * Rx(phi) * Ry(theta), then divided by its norm, then negated as a whole if w < 0: the yaw turns the robot
 *   about the WORLD's z axis, roll and pitch follow about the BODY's x and y axes.  (Rz(psi) = (0, 0, sin psi/2, cos psi/2) in the
 *   row's x, y, z, w order.)
 * Placing, if place_on_ground != 0: zmin = the smallest z of the support points of the robot's collision primitives on the NEW row
 *   (solorl_env_kin.prim_point[p][2], by the code solorl_kinematics runs; p = 0..19 on a Solo8, 0..23 on a Solo12; a NaN point is
 *   skipped);  pos.z <- pos.z + (clearance - zmin), up or down.  pos.x and pos.y are never written: a treadmill strip and a pointgoal
 *   potential stay valid.
 * Contact cache: lambda_prev[0..23] <- 0 and bits 0..23 of contact_mask <- 0 (bits 24.. and rng_counter keep their bits) if and only if
 *   the pose can change: some joint_pos[j], j < act_dim, or yaw, roll or pitch is non-zero, or place_on_ground is set.  (An impulse
 *   cached for a primitive that has moved is wrong.)  The four feet words of the next observation therefore read 0 until the first step.
 * Rows:
 *   selected   words pos .. qd (the first 37), and with the contact cache the 24 lambda_prev words and the contact_mask word, are
 *              written; no other word of the row is.  A non-finite member gives non-finite members of that row only; no index is
 *              computed from a row's data.
 *   masked (mask byte 0)   nothing of the row and not count[i] is read or written
 * Null cfg, p, rows or count, n < 1, a robot that is neither SOLORL_ROBOT_*, a negative or non-finite half-width or clearance, yaw, roll
 * or pitch above pi, a negative or non-finite cfg->joint_limit: SOLORL_ERR_INVALID, the message starts with "solorl_randomize_reset:"
 * (checked before any HIP call).
 * Shards: keyed by global env id: W batches of n rows at offsets k n draw like one batch of W n rows. */
typedef struct solorl_reset_randomization {
  uint64_t seed; int64_t env_id_offset;
  double joint_pos[12];   /* q[j]  += U(-a, a) [rad], then clamped to +-cfg->joint_limit */
  double joint_vel[12];   /* qd[j] += U(-a, a) [rad/s] */
  double lin_vel[3], ang_vel[3];   /* world frame, += U(-a, a) */
  double yaw, roll, pitch;         /* half-widths [rad] of the rotations above, each <= pi */
  double clearance;       /* [m] height of the lowest support point above z = 0 after placing */
  int32_t place_on_ground, reserved;
} solorl_reset_randomization;
int solorl_randomize_reset(const solorl_config* cfg, const solorl_reset_randomization* p,
                           solorl_env_state* rows /* [n] DEVICE rows, changed in place */,
                           const uint8_t* mask /* [n] or NULL */, uint32_t* count /* [n] device, in/out */, int n,
                           int device_id, void* stream);

/* solorl_restart_history: for the envs whose mask byte is non-zero, every history level the handle uses (0 .. num_history_stack - 1)
 * <- the observation words of the state the env holds NOW (SoloBase.get_current_state), in the engine's own arithmetic type, and then
 * -- if obs_out is not NULL -- the env's observation row, whose delta words are therefore exactly 0 and whose first D words equal
 * solorl_get_observation's.  Nothing else of the env and nothing of an unselected env is read or written; with contact-count sorting the
 * mask is read through the slot -> env map, as in solorl_reset_masked.  One launch on `stream`, no host synchronisation (capturable).
 * This is what a caller who writes q (or anything else the observation holds) with solorl_set_states needs instead of rebuilding the
 * HISTORY group on the host: see the JOINT_POS remark there.  Null handle or mask: SOLORL_ERR_INVALID, the message names the function;
 * SOLORL_ERR_STATE on a handle that has not been reset. */
int solorl_restart_history(solorl_env* env, const uint8_t* mask /* [N] device, not NULL */,
                           float* obs_out /* [N*O] or NULL */, void* stream);

/* Privileged critic rows (no reference counterpart; the "asymmetric actor-critic" of domain-randomised legged-robot training): the actor
 * keeps the observation row a robot could measure, the critic gets that row WITHOUT its sensor noise plus SOLORL_CRITIC_PRIV words of the
 * simulator's truth -- contact forces, foot heights and speeds, the command, the episode's progress, collisions, and what the actuation
 * and the kicks drew.  A sixth handle-free row query beside solorl_kinematics, solorl_dynamics, solorl_shape_reward, solorl_terminate
 * and solorl_randomize_reset: a pure function of its arguments, ONE kernel launch on `stream`, no allocation, no host synchronisation
 * (capturable).  E = p->obs_dim, A = the robot's 8 or 12 joints.  For every live row i:
 *   critic_out[i][0 .. E-1]  the bits of obs_in[i][0 .. E-1] (NaN payloads and -0.0 survive)
 *   critic_out[i][E + k]     (float)(raw_k * p->scale[k]), the product rounded in double first; raw_k in fp64:
 *    k       raw_k
 *    0..3    F_f: the normal force of foot f = FL, FR, HL, HR in the last sub-step [N] -- solorl_env_kin's prim_force of the foot
 *            primitive 13 + 2 f (the same functions compute it, and p_f and u_f below, from states[i])
 *    4..7    p_f.z: the height of that primitive's support point [m] (prim_point)
 *    8..11   sqrt(u_f.x * u_f.x + u_f.y * u_f.y): the horizontal speed of that point (prim_vel), each product rounded, then the sum
 *    12..14  cmd[i].cmd[0..2] (0 if cmd is NULL)
 *    15      states[i].timestep
 *    16      the number of set contact_mask bits among the robot's primitives other than the four foot primitives (term 13 of the
 *            shaped reward)
 *    17      act[i].latency (0 if act is NULL)
 *    18      ((g_0 + g_1) + ... + g_{A-1}) / A - 1 over act[i].gain[0 .. A-1], each widened to double, summed left to right (0 if act is NULL)
 *    19      sqrt(kick[i][0] * kick[i][0] + kick[i][1] * kick[i][1]), each product rounded, then the sum (0 if kick is NULL)
 *   Nothing is done about non-finite values: they propagate into the words they feed and into no other.
 * masked (mask byte 0): nothing of the row is read or written, in any array.  critic_out must not overlap obs_in.
 * Null cfg, p, states, obs_in or critic_out, n < 1, a robot that is neither SOLORL_ROBOT_*, obs_dim < 1 or > 210, a scale that is not
 * finite: SOLORL_ERR_INVALID, the message starts with "solorl_critic_obs:" (checked before any HIP call). */
#define SOLORL_CRITIC_PRIV 20
typedef struct solorl_critic_params {
  double scale[SOLORL_CRITIC_PRIV];   /* finite; 0 = that word reads 0 (or NaN where raw_k is not finite) */
  int32_t obs_dim;                    /* E: width of obs_in's rows; 1 <= E <= 210 */
  int32_t reserved;
} solorl_critic_params;
int solorl_critic_obs(const solorl_config* cfg, const solorl_critic_params* p,
                      const solorl_env_state* states /* [n] DEVICE rows: the state the observation describes */,
                      const uint8_t* mask /* [n] or NULL */, int n,
                      const float* obs_in /* [n][E]: the engine's clean observation rows */,
                      const solorl_env_command* cmd /* [n] rows or NULL */,
                      const solorl_env_actuator* act /* [n] rows or NULL */,
                      const double* kick /* [n][6] as solorl_perturb writes kick_out, or NULL */,
                      float* critic_out /* [n][E + SOLORL_CRITIC_PRIV] */, int device_id, void* stream);

/* Fused return computation over a rollout of T steps x N envs (device arrays, time-major [t][n]).
 * use_gae != 0:  value_preds[T][:] = next_value;  delta_t = r_t + gamma V_{t+1} m_{t+1} - V_t;
 *                A_t = delta_t + gamma lambda m_{t+1} A_{t+1};  returns[t] = A_t + V_t      (storage.py:41-50)
 * use_gae == 0:  returns[T][:] = next_value;  returns[t] = returns[t+1] gamma m_{t+1} + r_t   (storage.py:51-55) */
int solorl_compute_returns(const float* rewards /* [T*N] */, float* value_preds /* [(T+1)*N] */,
                           const float* masks /* [(T+1)*N] */, const float* next_value /* [N] */,
                           float* returns /* [(T+1)*N] */, int T, int N, int use_gae, float gamma,
                           float gae_lambda, int device_id, void* stream);

/* The same with time-limit bootstrapping: an episode the time limit ended is cut off, not finished, and its last return must not read
 * as that of a fall.  `timeouts` [T*N] are the bytes the step kernels write to solorl_info_soa.timeout, row t = the step that filled
 * rewards[t]; a byte is consulted only where masks[t+1] == 0 ("valid where done"), elsewhere its value does not matter.
 * With m = masks[t+1], V_t = value_preds[t] and  tl = (m == 0 && timeouts[t] != 0):
 * use_gae != 0:  value_preds[T][:] = next_value;  delta_t = r_t + gamma (tl ? V_t : V_{t+1} m) - V_t;
 *                A_t = delta_t + gamma lambda m A_{t+1};  returns[t] = A_t + V_t
 * use_gae == 0:  returns[T][:] = next_value;  returns[t] = r_t + gamma (tl ? V_t : returns[t+1] m)
 * A truncated step bootstraps from the value of the observation its action was taken from: that value is in the rollout already,
 * while the episode's true last observation was overwritten by the auto-reset inside the step kernel.  This is the rsl_rl /
 * legged_gym form (reward += gamma * value * time_out), not the bootstrap from the successor state.  The advantage chain is cut at
 * every episode end, truncated or not.
 * Where tl is false the arithmetic is solorl_compute_returns', expression for expression: with no truncation in the rollout the two
 * calls write the same bits (returns, and the row value_preds[T]).  One launch, one thread per env, 17 bytes per sample (16 without GAE).
 * Null array (timeouts too: a caller without flags calls solorl_compute_returns), T < 1 or N < 1: SOLORL_ERR_INVALID, the message
 * starts with "solorl_compute_returns_tl:" (checked before any HIP call). */
int solorl_compute_returns_tl(const float* rewards /* [T*N] */, float* value_preds /* [(T+1)*N] */,
                              const float* masks /* [(T+1)*N] */, const uint8_t* timeouts /* [T*N] */,
                              const float* next_value /* [N] */, float* returns /* [(T+1)*N] */,
                              int T, int N, int use_gae, float gamma, float gae_lambda, int device_id, void* stream);

/* Running normalisation of observations and rewards (VecNormalize, agents/running_mean_std.py:73-127).  State is the caller's device
 * memory: `stats` = mean[D], var[D], count as 2 D + 1 doubles (initially 0, 1, 1e-4: running_mean_std.py:13-16; D = the observation size,
 * or 1 for the returns) and `ret` = the n discounted-return accumulators, doubles as the reference's.  Statistics and batch moments are
 * fp64 sums in an order that depends on (n, D) only -- no atomics, the same bits on every run and graph replay, and one call over R rows
 * gives the bits of R calls over one row; outputs are rounded to float once.  Everything is enqueued on `stream` as a linear chain of
 * launches whose number does not depend on `rows` (update != 0: 4 for observations, 5 for rewards; update == 0: one), without host
 * synchronisation or allocation: capturable.  Limits: D <= 1024, rows <= 65535, n D < 2^31, a scratch count below 2^31.
 * Null array, `rows`, `n` or `D` < 1, a shape beyond the limits or a null `scratch`: SOLORL_ERR_INVALID, the message names the function
 * (checked before any HIP call). */

/* doubles of scratch the two calls below need with these (rows, n, D) -- D = 1 for the rewards (0 for bad arguments) */
int solorl_norm_scratch_count(int rows, int n, int D);

/* VecNormalize._obfilt (running_mean_std.py:109-116) for rows x [n][D] observations, row after row:
 *   update != 0: stats <- update_mean_var_count_from_moments of (stats, mean_n x, var_n x, n)   (:18-39; population variance)
 *   out = clip((x - mean) / sqrt(var + epsilon), -clip, clip)   with the stats AFTER that row's update
 * obs_out may be obs_in (in place). */
int solorl_normalize_obs(double* stats, int rows, int n, int D, const float* obs_in, float* obs_out,
                         int update, double clip, double epsilon, double* scratch, int device_id, void* stream);

/* VecNormalize.step's reward half (:98-105) for rows x [n] rewards, row after row:
 *   ret = ret * gamma + r;  update != 0: stats (D = 1) <- moments of ret over the n envs;
 *   r_out = clip(r / sqrt(var + epsilon), -clip, clip);  ret[done != 0] = 0          (in this order)
 * rewards are rewritten in place; done is [rows][n] bytes. */
int solorl_normalize_rewards(double* stats, double* ret, int rows, int n, float* rewards, const uint8_t* done,
                             int update, double gamma, double clip, double epsilon, double* scratch,
                             int device_id, void* stream);

/* Fused PPO mini-batch loss, forward + gradients w.r.t. the policy heads (device arrays, m samples, A action dims):
 *   logp_i = sum_j -0.5 z_ij^2 - logstd_j - log sqrt(2 pi),  z = (action - mean) exp(-logstd);  ratio = exp(logp - old_logp)
 *   action loss = -mean_i min(ratio adv, clamp(ratio, 1-clip, 1+clip) adv)                                  (ppo.py:54-59)
 *   value  loss = 0.5 mean_i max((v - ret)^2, (vpred + clamp(v - vpred, +-clip) - ret)^2)  [clipped_value]  (ppo.py:61-68)
 * Outputs: grad_mean [m*A] = d(action loss)/d mean, grad_values [m] = value_coef * d(value loss)/d v, and per-block
 * partial sums partials[ceil(m/256)][3 + A] = (sum value loss, sum action loss, count, d(action loss)/d logstd[A]);
 * the caller adds the blocks (deterministic) and the entropy term, which does not depend on the samples. */
int solorl_ppo_loss(const float* mean, const float* logstd, const float* values, const float* action, const float* old_logp,
                    const float* adv, const float* vpred, const float* ret, int m, int A, float clip, float value_coef,
                    int clipped_value, float* grad_mean, float* grad_values, float* partials, int device_id, void* stream);

/* Parameters of the reference's MLP actor-critic in PyTorch layout (nn.Linear weight = [out][in], row-major), device pointers:
 * base.critic.{0,2,4}, base.features.{0,2}, pi_dist.mean, pi_dist.logstd (agents/ppo/policy.py:62-81,138-148).  The kernels
 * are built for hidden = 64 and (obs_dim, act_dim) in {(38|42|76|84, 12), (30|34|60|68, 8)} -- zero or one history level -- and
 * {(41|45, 12), (33|37, 8)} -- zero history levels with the three command words of solorl_commands; other shapes
 * return SOLORL_ERR_INVALID and the caller keeps its framework path.  Alignment: the weight matrices critic_w1/w2, actor_w1,
 * mean_w -- and, when obs_dim % 4 == 0, critic_w0, actor_w0 and every `obs` array handed to solorl_policy_act /
 * solorl_ppo_batch -- are read as float4 rows and must start on a 16-byte boundary (checked: SOLORL_ERR_INVALID otherwise).
 * The same table goes to the width-generic family (the _w entry points at the end of this header), which takes hidden = 64,
 * act_dim 8 or 12 and ANY obs_dim and critic_obs_dim up to SOLORL_POLICY_MAX_WIDTH, the shapes above included. */
#define SOLORL_POLICY_MAX_WIDTH 128
typedef struct solorl_policy_params {
  int obs_dim, act_dim, hidden;
  int critic_obs_dim;   /* 0: the critic reads the actor's rows (symmetric); OC != 0: critic_w0 is [64][OC] and the critic reads rows of OC
                         * words of its own (the slot was reserved0: size and layout are unchanged) */
  const float *critic_w0, *critic_b0, *critic_w1, *critic_b1, *critic_w2, *critic_b2;
  const float *actor_w0, *actor_b0, *actor_w1, *actor_b1, *mean_w, *mean_b, *logstd;
} solorl_policy_params;

/* Policy.act for n observation rows: value_out[n], action_out[n][A] = mean + exp(logstd) * noise (noise[n][A]: the caller's
 * standard-normal draw; NULL = deterministic, action = mean), logp_out[n] = log N(action; mean, exp(logstd)) summed over A. */
int solorl_policy_act(const solorl_policy_params* p, const float* obs /* [n][obs_dim] */, const float* noise, int n, float* value_out,
                      float* action_out, float* logp_out, int device_id, void* stream);

/* One PPO mini-batch, everything of forward + backward except the weight-gradient GEMMs.  Sample r of the mini-batch is
 * row perm[*offset + r] of the rollout arrays (perm, offset: device memory, so a captured launch needs no host argument). */
typedef struct solorl_ppo_batch {
  const float *obs /* [n][obs_dim] */, *actions /* [n][A] */, *old_logp, *adv, *vpred, *ret /* [n] each */;
  const int64_t *perm, *offset;
  int m;                       /* mini-batch rows */
  int clipped_value;           /* ppo.py:61 use_clipped_value_loss */
  float clip, value_coef;      /* ppo.py:56 clip_param; the value-loss coefficient is folded into the critic's gradient */
} solorl_ppo_batch;
/* Outputs (m a multiple of 32), each units x m floats laid out [tile = row / 32][unit][row % 32] -- a tile of 32 rows is one contiguous
 * block (ABI 5; it was [unit][m]): xt0 = gathered observations (obs_dim units); per net (c_ critic, a_ actor) the hidden activations
 * xt1, xt2 (64 units), the pre-activation gradients g1, g2 (64 units) and the head-output gradient gh (1 / A units).
 * Weight gradients are then G X^T products over the rows:  d W0 = g1 xt0^T, d W1 = g2 xt1^T, d Whead = gh xt2^T, biases = row
 * sums of g.  partials [m / 32][3 + A]: per 32 rows (sum value loss, sum action loss, rows, sum d action-loss / d logstd_a; ABI 5:
 * one row per 32 samples, it was 64);
 * the entropy term of ppo.py:74 does not depend on the samples and is left to the caller. */
typedef struct solorl_ppo_stage1 {
  float *xt0, *c_xt1, *c_xt2, *c_g1, *c_g2, *c_gh, *a_xt1, *a_xt2, *a_g1, *a_g2, *a_gh, *partials;
} solorl_ppo_stage1;
int solorl_ppo_grad_stage1(const solorl_policy_params* p, const solorl_ppo_batch* batch, const solorl_ppo_stage1* work, int device_id,
                           void* stream);

/* Stage 2: the weight gradients d W = g x^T (+ biases) of all six layers from stage 1's arrays, and the step's bookkeeping.
 * `out` names where each gradient goes (PyTorch layouts, e.g. views of one flat bucket), plus
 *   loss_sums [3 + A]  += (sum value loss, sum action loss, rows, sum d action-loss / d logstd) of this mini-batch,
 *   logstd_sum [1]     += sum_a logstd_a            (entropy = 0.5 + log sqrt(2 pi) + mean_a logstd_a, policy.py:56)
 *   logstd             = sum d action-loss / d logstd - entropy_coef / A       (the complete gradient of ppo.py:74's loss)
 *   scratch            >= solorl_ppo_scratch_count(obs_dim, act_dim, m) floats of working memory (one solorl_ppo_grad_count block per
 *                      chunk of rows; ABI 5 cut the rows into ~170 chunks instead of ceil(m / 512)).
 * Sums are taken in a fixed order: results are reproducible run to run. */
typedef struct solorl_ppo_grads {
  float *critic_w0, *critic_b0, *critic_w1, *critic_b1, *critic_w2, *critic_b2;
  float *actor_w0, *actor_b0, *actor_w1, *actor_b1, *mean_w, *mean_b, *logstd;
  float *loss_sums, *logstd_sum, *scratch;
  float entropy_coef, reserved0;
} solorl_ppo_grads;
int solorl_ppo_grad_stage2(const solorl_policy_params* p, const solorl_ppo_stage1* work, int m, const solorl_ppo_grads* out, int device_id,
                           void* stream);
/* number of weight + bias elements of the actor-critic except logstd (one scratch chunk) */
int solorl_ppo_grad_count(int obs_dim, int act_dim);
/* floats of solorl_ppo_grads.scratch that solorl_ppo_grad_stage2 needs for a mini-batch of m rows (0 for m < 1) */
int solorl_ppo_scratch_count(int obs_dim, int act_dim, int m);

/* Gradient-norm clip + Adam step over the 13 parameter tensors in one launch: nn.utils.clip_grad_norm_(max_grad_norm)
 * (agents/ppo/ppo.py:75-76; coefficient max_norm / (norm + 1e-6) clamped to 1) followed by torch.optim.Adam's update (:32, :77:
 * bias-corrected, eps outside the square root, L2 weight_decay added to the gradient, no amsgrad).  The parameters behind `p`
 * are UPDATED IN PLACE; exp_avg / exp_avg_sq hold solorl_ppo_grad_count(obs_dim, act_dim) + act_dim floats in the order of
 * solorl_policy_params' pointers; step [1] is incremented; lr [1] is read from the device (a schedule may rewrite it between
 * calls); offset (optional) is advanced by offset_increment -- the mini-batch cursor of solorl_ppo_batch.  grad_scale folds the
 * 1 / world_size of a data-parallel gradient mean into the same launch. */
typedef struct solorl_adam_state {
  float *exp_avg, *exp_avg_sq, *step;
  const float* lr;
  int64_t* offset;
  int64_t offset_increment;
  float beta1, beta2, eps, weight_decay, max_grad_norm /* <= 0: no clipping */;
  float grad_scale;   /* every gradient element is multiplied by this before the norm and the update: 1 / world_size after a SUMMED
                       * all-reduce of the flat bucket (data-parallel mean); <= 0 is read as 1 */
} solorl_adam_state;
int solorl_ppo_clip_adam(const solorl_policy_params* p, const solorl_ppo_grads* g, const solorl_adam_state* a, int device_id, void* stream);

/* solorl_step followed by Policy.act (agents/ppo/policy.py:33-49) on the NEW observation of every env, in the same launch: value_out
 * [N], action_out [N][A] = mean + exp(logstd) * noise (noise [N][A]: the caller's standard-normal draw; NULL: action = mean),
 * logp_out [N].  What the reference's rollout loop does with two calls per step (agents/ppo/train.py:84-88) and solorl_policy_act +
 * solorl_step do with two launches.  Why one: at 4096 envs per GPU the step launch lasts as long as its slowest wavefront while the
 * mean wavefront is done in half that time; each wavefront evaluates the policy for its own four envs as soon as their observations
 * exist, so the policy costs no launch of its own.  Needs the engine's defaults (fp32, team mode, no contact-count sorting), hidden
 * = 64, obs_dim = this env's observation size, a multiple of 4 and at most 88 (zero or one history level), 16-byte aligned weight matrices; otherwise
 * SOLORL_ERR_INVALID and the caller keeps the two-call form.  Outputs equal solorl_policy_act's on the same rows up to the order
 * of the f32 sums (tested: 2e-6). */
int solorl_step_act(solorl_env* env, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out,
                    const solorl_info_soa* info_out, const solorl_policy_params* p, const float* noise, float* value_out,
                    float* action_out, float* logp_out, void* stream);

/* K control steps = K calls of solorl_step, in one launch where solorl_get_property "step_n_one_launch" is 1 (the defaults: team
 * mode, no contact-count sorting; otherwise the engine issues K ordinary steps itself, with the same results).  One launch: each
 * wavefront runs its own four envs through all K steps without waiting for the others in between, so a window costs about the sum
 * of the MEAN wavefront's steps instead of K times the slowest one's.
 * actions [K][N][A]; obs_out [K][N][O]; reward_out [K][N]; done_out [K][N];
 * info_out: every per-step field is [K][N] (applied_torque [K][N][A]); ep_stats stays [FIELDS][N] and accumulates.
 * K < 1 or a null array: SOLORL_ERR_INVALID; before reset: SOLORL_ERR_STATE.  No host synchronisation, no allocation (capturable). */
int solorl_step_n(solorl_env* env, int K, const float* actions, float* obs_out, float* reward_out, uint8_t* done_out,
                  const solorl_info_soa* info_out, void* stream);

/* Closed loop = K calls of solorl_step_act, the action each produces driving the next step, in one launch.
 * Rows are rollout-storage rows: row r of actions / noise / value_out / logp_out belongs to the observation produced by step r-1.
 * actions: row 0 is read; rows 1..K-1 are written, and row K too when policy_after_last != 0 (the first action of the next
 * window; the caller then provides K + 1 rows of actions, noise, value_out and logp_out).  Row 0 of noise / value_out / logp_out is
 * neither read nor written; noise NULL: every action = the mean.  Other outputs as solorl_step_n.
 * Same prerequisites as solorl_step_act, otherwise SOLORL_ERR_INVALID. */
int solorl_rollout(solorl_env* env, int K, float* actions, float* obs_out, float* reward_out, uint8_t* done_out,
                   const solorl_info_soa* info_out, const solorl_policy_params* p, const float* noise,
                   float* value_out, float* logp_out, int policy_after_last, void* stream);

/* The asymmetric actor-critic (privileged critic): a policy whose solorl_policy_params.critic_obs_dim = OC != 0 -- the critic's first layer
 * is [64][OC] and reads rows of its own, e.g. solorl_critic_obs' -- goes through the three entry points below, which are the ones above
 * with the critic's rows beside the actor's; the ones above refuse such a policy (SOLORL_ERR_INVALID).  Built for (obs_dim, OC, act_dim) =
 * (38, 58, 12), (41, 58, 12), (76, 96, 12), (30, 50, 8), (33, 50, 8), (60, 80, 8): walk and stand at zero and one history level and the
 * commanded zero-history widths, OC = the engine's width + SOLORL_CRITIC_PRIV; other shapes return SOLORL_ERR_INVALID and the caller
 * keeps its framework path.  solorl_ppo_clip_adam reads both widths from p and serves both forms.
 *   solorl_policy_act_critic       value_out from critic_obs [n][OC], action_out and logp_out from obs [n][obs_dim]
 *   solorl_ppo_grad_stage1_critic  critic_obs [rows][OC]: the rollout's critic rows, gathered through batch->perm like batch->obs;
 *                                  work->xt0 receives the ACTOR's gathered rows (obs_dim units), critic_xt0 (OC x m floats, tiled like
 *                                  xt0) the critic's
 *   solorl_ppo_grad_stage2_critic  the critic's first layer from critic_xt0 with K = OC; out->scratch holds
 *                                  solorl_ppo_scratch_count2 floats, the moments of solorl_adam_state solorl_ppo_grad_count2 + act_dim
 * Rows of a width that is a multiple of 4 (and critic_w0 when OC is) must start on a 16-byte boundary. */
int solorl_policy_act_critic(const solorl_policy_params* p, const float* obs /* [n][obs_dim] */, const float* critic_obs /* [n][OC] */,
                             const float* noise, int n, float* value_out, float* action_out, float* logp_out, int device_id, void* stream);
int solorl_ppo_grad_stage1_critic(const solorl_policy_params* p, const solorl_ppo_batch* batch, const float* critic_obs,
                                  const solorl_ppo_stage1* work, float* critic_xt0, int device_id, void* stream);
int solorl_ppo_grad_stage2_critic(const solorl_policy_params* p, const solorl_ppo_stage1* work, const float* critic_xt0, int m,
                                  const solorl_ppo_grads* out, int device_id, void* stream);
int solorl_ppo_grad_count2(int obs_dim, int critic_obs_dim, int act_dim);
int solorl_ppo_scratch_count2(int obs_dim, int critic_obs_dim, int act_dim, int m);

/* The width-generic family: the same four steps for hidden = 64, act_dim 8 or 12 and any 1 <= obs_dim <= SOLORL_POLICY_MAX_WIDTH,
 * critic_obs_dim = 0 (symmetric) or 1 .. SOLORL_POLICY_MAX_WIDTH other than obs_dim; anything else is SOLORL_ERR_INVALID with a message that
 * names the cap.  The widths are run-time values of ONE kernel per action width instead of a template instance per shape, and every sum is
 * taken in the order the per-shape kernels take it: at a shape those are built for, these write the same bits.  One set of entry points
 * serves both forms: critic_obs / critic_xt0 are NULL for the symmetric policy (critic_obs_dim = 0) and the critic's arrays, as in the
 * _critic entry points, for a policy with a critic width; given with critic_obs_dim = 0, or missing with one set, they are refused.
 * Working memory and moments are sized by solorl_ppo_scratch_count2 / solorl_ppo_grad_count2 with the critic's width (obs_dim for the
 * symmetric policy).  Alignment, the multiples of 32 / 64 rows and the 32-bit bound on m x width are those of the entry points above. */
int solorl_policy_act_w(const solorl_policy_params* p, const float* obs /* [n][obs_dim] */, const float* critic_obs /* [n][OC] or NULL */,
                        const float* noise, int n, float* value_out, float* action_out, float* logp_out, int device_id, void* stream);
int solorl_ppo_grad_stage1_w(const solorl_policy_params* p, const solorl_ppo_batch* batch, const float* critic_obs,
                             const solorl_ppo_stage1* work, float* critic_xt0, int device_id, void* stream);
int solorl_ppo_grad_stage2_w(const solorl_policy_params* p, const solorl_ppo_stage1* work, const float* critic_xt0, int m,
                             const solorl_ppo_grads* out, int device_id, void* stream);
int solorl_ppo_clip_adam_w(const solorl_policy_params* p, const solorl_ppo_grads* g, const solorl_adam_state* a, int device_id, void* stream);

/* PPO KL control on the device: the approximate KL divergence and the clip fraction of every mini-batch step, a learning rate that
 * follows the KL (rsl_rl's "adaptive" schedule) and an early stop of the update (stable-baselines' target_kl), without a launch more
 * and without a host round trip -- capturable like the steps they stand in for.  No struct above changes (SOLORL_ABI_VERSION stays).
 *
 * solorl_ppo_grad_stage1_kl is stage 1 with one more output: diag [m / 32][2], per tile of 32 rows the sums over its rows of
 *   k3 = (ratio - 1) - (logp - old_logp)      Schulman's estimator of KL(old || new) (stable-baselines' approx_kl), >= 0 per row
 *   1 - inside                                 1 for a row whose ratio left [1 - clip, 1 + clip]
 * Every other output has the bits the plain entry point writes.  Stage 2 follows unchanged.
 *
 * solorl_ppo_clip_adam_kl is clip + Adam with the controller in front.  It adds diag up in a fixed order, kl = sum k3 / m and
 * cf = sum (1 - inside) / m, and then, in f32 and in this order:
 *   1. target_kl > 0 and kl > 1.5 target_kl                     the stopped flag state[4] is set, and stays set until the caller clears it
 *   2. not stopped and desired_kl > 0:
 *        kl > 2 desired_kl                                      lr = max(lr_min, lr / lr_factor)
 *        else kl < desired_kl / 2 and kl > 0                    lr = min(lr_max, lr * lr_factor)
 *      and lr is written back to *lr and used by this step
 *   3. stopped: no parameter, moment or step count is written; the cursor a->offset still advances
 * A kl that is not finite decides nothing: no stop, no change.  With desired_kl <= 0 and target_kl <= 0 and a clear flag the
 * parameters, moments, step count and cursor are bit for bit solorl_ppo_clip_adam's.
 *   state [8]   += (1, applied ? 1 : 0, kl, cf) in [0..3]; [4] the stopped flag; [5..7] = this step's kl, cf and lr.  The caller zeroes it
 *               at the start of an update.
 *   log         optional [log_capacity][4]: row state[0] (the steps seen before this one), while below log_capacity, receives
 *               (kl, cf, the lr used, 1 if the step was applied else 0)
 *   lr          must be a->lr; m the mini-batch's rows (= a->offset_increment where a->offset is given)
 * One pair of entry points serves the three kernel families: generic != 0 picks the width-generic kernels (the _w entry points'
 * shapes), 0 the kernels built per shape; critic_obs / critic_xt0 go with p->critic_obs_dim as in the _w entry points (NULL for a
 * symmetric policy).  Refused with SOLORL_ERR_INVALID, before the device is looked up and with a message that starts with the
 * entry point's name: what the plain entry points refuse; a null diag, state or lr; lr other than a->lr; m that is not the
 * batch's; lr_factor <= 1; lr_min > lr_max. */
typedef struct solorl_kl_control {
  const float* diag;   /* [m / 32][2], written by solorl_ppo_grad_stage1_kl */
  int m;
  float desired_kl, lr_factor, lr_min, lr_max, target_kl;
  float* lr;
  float* state;
  float* log;
  int log_capacity;
} solorl_kl_control;
int solorl_ppo_grad_stage1_kl(const solorl_policy_params* p, const solorl_ppo_batch* batch, const float* critic_obs,
                              const solorl_ppo_stage1* work, float* critic_xt0, float* diag, int generic, int device_id, void* stream);
int solorl_ppo_clip_adam_kl(const solorl_policy_params* p, const solorl_ppo_grads* g, const solorl_adam_state* a,
                            const solorl_kl_control* k, int generic, int device_id, void* stream);

const char* solorl_last_error(void);
const char* solorl_version(void);
int solorl_abi_version(void);   /* SOLORL_ABI_VERSION of the built library */

#ifdef __cplusplus
}
#endif
#endif /* SOLORL_H */
