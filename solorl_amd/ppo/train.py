"""PPO training loop over the HIP rollout engine -- `train(args, config, env_constructor, writer)`
with the argument meaning of the reference's agents/ppo/train.py:21-162 and the flags of
training/train_ppo.py:9-45.

Differences that come with the GPU engine (documented, not behavioural):
  * rollout, policy forward, storage and update all stay on one HIP device: no device->host->pickle
    ->Pipe round trip per step (agents/ppo/envs.py:189-196);
  * episode statistics are accumulated by the step kernel on the device at EVERY step (no sampling) instead of
    iterating N Python dicts per step (train.py:90-100) -- same quantities: episode_reward (last-step reward,
    baseEnv.py:65), episode_length, success, dr/* sums, as means over the episodes finished per log interval;
  * args.normalize_obs / args.normalize_returns switch on the reference's VecNormalize (agents/running_mean_std.py:73-127; its launcher
    hard-codes both off) on the device, single process only; the checkpoint's `ob_rms` then carries the statistics, as the reference's;
  * args.push_interval / args.push_max_vel / args.push_max_yaw_rate (train_ppo.py --push-interval LO[:HI] ...; no reference counterpart)
    kick every training env's base at random intervals, drawn and applied on the device in front of every step launch of the eager
    and of the captured rollout alike (SoloVecEnv.set_perturbation); the schedule is keyed by global env id, so ranks kick like one batch;
  * args.reward_shaping (train_ppo.py --reward-shaping FILE.yaml: a dict with `weights` and the terms' parameters; no reference
    counterpart) adds shaped reward terms behind every step launch of the eager and of the captured rollout alike
    (SoloVecEnv.set_reward_shaping); each term's weighted sum per finished episode is logged as sr/<name> beside dr/*;
  * args.obs_noise / args.action_delay / args.motor_gain_range (train_ppo.py --obs-noise FILE.yaml --action-delay LO[:HI]
    --motor-gain-range G; no reference counterpart) put uniform sensor noise on every observation the rollout stores and the policy reads,
    and actuation latency with a per-joint motor gain error between the stored raw actions and the engine, in the eager and in the
    captured rollout alike (SoloVecEnv.set_obs_noise / set_actuation); both are keyed by global env id, so ranks draw like one batch.
    With noise the policy cannot run inside the step kernel (it would read clean observations): the rollout takes two launches per step;
  * args.commands (train_ppo.py --commands FILE.yaml: a dict of ranges; no reference counterpart) gives every env a velocity command of
    its own, drawn and resampled on the device behind every step launch of the eager and of the captured rollout alike
    (SoloVecEnv(commands=)): the observation and the policy are three words wider, and the tracking terms of args.reward_shaping compare
    each env against its own command.  The policy cannot run inside the step kernel either (it would not see the command words);
  * args.termination (train_ppo.py --termination FILE.yaml: a dict of rules; no reference counterpart) ends an episode early when the
    state after a step breaks a rule -- base height, tilt, contact of chosen primitives, joint limits -- by one launch behind every
    step launch of the eager and of the captured rollout alike (SoloVecEnv.set_termination), the envs it ends reset on the device; the
    share of the finished episodes each rule ended is logged as term/<rule> beside dr/* and sr/*.  The policy cannot run inside the step
    kernel (it would act on the observation of an env that is about to be reset): the rollout takes two launches per step;
  * args.reset_randomization (train_ppo.py --reset-randomization FILE.yaml: a dict of half-widths; no reference counterpart) starts every
    episode from a randomised state -- joint angles and velocities, base velocity, heading, roll and pitch, the robot placed on the
    ground -- by four launches behind every step launch of the eager and of the captured rollout alike
    (SoloVecEnv.set_reset_randomization), keyed by global env id, so ranks draw like one batch.  The policy cannot run inside the step
    kernel (it would act on the observation of the un-randomised reset): the rollout takes two launches per step;
  * args.privileged_critic (train_ppo.py --privileged-critic [FILE.yaml]: True, or a dict of scales; no reference counterpart) gives the
    value function rows of its own -- the observation before the sensor noise plus twenty words of the simulator's truth, written by
    two launches behind every step launch of the eager and of the captured rollout alike (SoloVecEnv(critic_obs=)) -- while the actor
    keeps the row a robot could measure: Policy(critic_obs_dim=), RolloutStorage(critic_obs_dim=).  No policy kernel is built at a
    critic width, so the rollout's act and the mini-batch step take their PyTorch paths (inside the same HIP graphs);
  * args.bootstrap_timeouts (train_ppo.py --bootstrap-timeouts; no reference counterpart: its returns treat an episode the time limit
    ended like a fall) keeps the engine's timeout flag of every step in the rollout storage -- written there by the step launches
    themselves, of the eager and of the captured rollout alike (SoloVecEnv.step_inplace(timeout_out=)) -- and computes the returns
    with solorl_compute_returns_tl: a truncated step bootstraps from the value of the observation its action was taken from;
  * multi-GPU: one process per GPU (`python -m torch.distributed.run --nproc-per-node W ...`), envs
    sharded by rank (global env id = rank*N + i), flat-bucket RCCL gradient all-reduce (ppo.py).
"""
import os
import time

import torch

from . import dist as D
from .policy import Policy
from .ppo import PPO
from .graphs import GraphedPPO, GraphedRollout
from .storage import RolloutStorage


def update_linear_schedule(optimizer, epoch, total_num_epochs, initial_lr):
    """agents/utils.py:14-18: lr decays linearly to zero."""
    lr = initial_lr - (initial_lr * (epoch / float(total_num_epochs)))
    for g in optimizer.param_groups:
        if torch.is_tensor(g["lr"]):      # capturable Adam (GraphedPPO): the graph reads the device tensor
            g["lr"].fill_(lr)
        else:
            g["lr"] = lr


def episode_stats(envs, device):
    """Means over ALL episodes finished since the last call (every step counts), from the engine's on-device
    accumulators (vec_env.SoloVecEnv.episode_stat_sums; include/solorl.h `ep_stats`), summed over ranks.  The
    reference keeps deques of the last 32 finished episodes (agents/ppo/train.py:66-70,90-100) and prints their
    mean; with thousands of envs the per-interval mean is the same quantity without the 32-episode window."""
    from ..config import EPSTAT_NAMES
    sums = envs.episode_stat_sums(reset=True)
    if D.world() > 1:
        import torch.distributed as dist
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    tot = sums.tolist()
    n = tot[0]
    out = {"episodes": int(n), "nan_resets": int(tot[9])}
    for k in range(1, 9):
        out[EPSTAT_NAMES[k]] = (tot[k] / n) if n > 0 else float("nan")
    return out


def rollout(envs, actor_critic, storage, num_steps):
    """train.py:82-103: T steps of act -> env.step -> storage.append, entirely on the device (the episode statistics
    of train.py:90-100 are accumulated by the step kernel itself)."""
    asym = storage.critic_obs is not None                 # an asymmetric policy: the critic reads the env's critic rows
    for step in range(num_steps):
        with torch.no_grad():
            value, action, logp = actor_critic.act(storage.obs[step], **({"critic_inputs": storage.critic_obs[step]} if asym else {}))
        obs, reward, done, info = envs.step_inplace(action.contiguous())
        storage.append(obs, action, logp, value, reward.unsqueeze(-1), (1.0 - done.float()).unsqueeze(-1),
                       **({"critic_obs": envs.last_critic_obs} if asym else {}),
                       **({"timeouts": info["timeout"]} if storage.timeouts is not None else {}))


def train(args, config, env_constructor=None, writer=None):
    from ..vec_env import make_vec_envs
    rank, world = D.init_from_env("cuda" if args.cuda else "cpu")
    torch.set_num_threads(1)                          # as the reference's learner (train.py:29); with one process per GPU the host work is a few scalars,
                                                      # and torch's default pool (one thread per host core) only competes with the other ranks
    torch.manual_seed(args.seed)                      # identical initial weights on every rank (train.py:23)
    if args.cuda:
        torch.cuda.manual_seed_all(args.seed)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0"))) if args.cuda else torch.device("cpu")
    N = args.num_agents
    norm_obs, norm_ret = bool(getattr(args, "normalize_obs", False)), bool(getattr(args, "normalize_returns", False))
    if world > 1 and (norm_obs or norm_ret):
        # every rank would keep statistics of its own shard and the policies would drift apart; merging moments across ranks is not built
        raise NotImplementedError("--normalize-obs / --normalize-returns need a single process (world size %d): the running statistics "
                                  "are not merged across ranks" % world)
    # PPO KL control (ppo/kl_control.py): --desired-kl, --target-kl, --ppo-diagnostics; all off: no argument more goes to the agent
    kl_args = {k: v for k, v in (("desired_kl", getattr(args, "desired_kl", None)), ("target_kl", getattr(args, "target_kl", None)),
                                 ("diagnostics", bool(getattr(args, "ppo_diagnostics", False)))) if v}
    if kl_args.get("desired_kl") and args.use_linear_lr_decay:
        raise ValueError("--desired-kl with --use-linear-lr-decay: two schedules for one learning rate")
    if world > 1 and kl_args:
        # the KL sums are per rank: the ranks would adapt different rates and stop at different steps
        raise NotImplementedError("--desired-kl / --target-kl / --ppo-diagnostics need a single process (world size %d): the KL sums "
                                  "are not merged across ranks" % world)
    envs = make_vec_envs(config, N, env_constructor, args.gamma, device, seed=args.seed, env_id_offset=rank * N,
                         norm_obs=norm_obs, norm_ret=norm_ret, push_interval=getattr(args, "push_interval", None),
                         push_max_vel=getattr(args, "push_max_vel", 0.0), push_max_yaw_rate=getattr(args, "push_max_yaw_rate", 0.0),
                         reward_shaping=getattr(args, "reward_shaping", None), obs_noise=getattr(args, "obs_noise", None),
                         action_delay=getattr(args, "action_delay", None), motor_gain_range=getattr(args, "motor_gain_range", 0.0),
                         commands=getattr(args, "commands", None), termination=getattr(args, "termination", None),
                         reset_randomization=getattr(args, "reset_randomization", None),
                         critic_obs=getattr(args, "privileged_critic", None) or None)
    shaping = getattr(args, "reward_shaping", None) is not None
    termination = getattr(args, "termination", None) is not None
    action_dim = envs.action_space.shape[0]
    base = torch.load(args.base_checkpoint) if getattr(args, "base_checkpoint", None) else None
    critic_dim = getattr(envs, "critic_obs_dim", None)    # None: the critic reads the actor's rows
    critic_of = (lambda t: {"critic_inputs": storage.critic_obs[t]}) if critic_dim is not None else (lambda t: {})
    actor_critic = Policy(envs.observation_space.shape, envs.action_space, base, {"hidden_size": args.hidden_size},
                          critic_obs_dim=critic_dim).to(device)
    D.broadcast_parameters(actor_critic)
    use_graphs = bool(args.cuda) and not getattr(args, "no_hip_graphs", False)
    agent = (GraphedPPO if use_graphs else PPO)(actor_critic, args.clip_param, args.ppo_epoch, args.mini_batch_size,
                                                 args.value_loss_coef, args.entropy_coef, lr=args.lr, l2_coef=args.l2_coef,
                                                 max_grad_norm=args.max_grad_norm, **kl_args)
    bootstrap = bool(getattr(args, "bootstrap_timeouts", False))
    storage = RolloutStorage(args.num_steps, N, envs.observation_space.shape, action_dim, device, critic_obs_dim=critic_dim,
                             bootstrap_timeouts=bootstrap)
    if bootstrap and rank == 0:
        print("time-limit bootstrapping on: a step the time limit cut off bootstraps from the value of its own observation "
              "(solorl_compute_returns_tl)", flush=True)
    storage.obs[0].copy_(envs.reset())
    if critic_dim is not None:
        storage.critic_obs[0].copy_(envs.last_critic_obs)
    torch.manual_seed(args.seed + 1000 * rank)        # but different action noise per rank
    if use_graphs:
        with torch.no_grad():
            actor_critic.act(storage.obs[0], **critic_of(0)); actor_critic.get_value(storage.obs[0], **critic_of(0))    # library workspaces before capture
        torch.manual_seed(args.seed + 1000 * rank)
        graphed_rollout = GraphedRollout(envs, actor_critic, storage, args.num_steps)
    start = time.time()
    num_updates = int(args.num_env_steps) // args.num_steps // (N * world)
    history = []
    for j in range(num_updates):
        if args.use_linear_lr_decay:
            update_linear_schedule(agent.optimizer, j, num_updates, args.lr)
        if use_graphs:
            graphed_rollout()
        else:
            rollout(envs, actor_critic, storage, args.num_steps)
        with torch.no_grad():
            next_value = actor_critic.get_value(storage.obs[-1], **critic_of(-1))
        storage.compute_returns(next_value, args.use_gae, args.gamma, args.tau)
        value_loss, action_loss, entropy = agent.update(storage)
        storage.reset()
        if getattr(args, "curriculum_schedule", 0) and (j + 1) % args.curriculum_schedule == 0:
            envs.increment_curriculum()
        total = (j + 1) * N * world * args.num_steps
        if rank == 0 and args.logdir is not None and (j % args.save_interval == 0 or j == num_updates - 1):
            os.makedirs(args.logdir, exist_ok=True)
            # ob_rms / ret_rms: host RunningMeanStd copies of the device statistics (one small device -> host copy each)
            ckpt = {"update": j, "state_dict": actor_critic.state_dict(), "ob_rms": getattr(envs.envs, "ob_rms", None)}
            if getattr(envs.envs, "ret_rms", None) is not None:
                ckpt["ret_rms"] = envs.envs.ret_rms
            torch.save(ckpt, os.path.join(args.logdir, "solo_{}.pt".format(total)))
            torch.save(ckpt, os.path.join(args.logdir, "solo.pt"))
        if j % args.log_interval == 0:
            es = episode_stats(envs, device)
            fps = int(total / (time.time() - start))
            rec = dict(update=j, timesteps=total, fps=fps, value_loss=value_loss, action_loss=action_loss, entropy=entropy,
                       ep_reward=es["episode_reward"], ep_length=es["episode_length"], success=es["success"],
                       episodes=es["episodes"], **{k: v for k, v in es.items() if k.startswith("dr/")})
            if shaping:                               # this rank's finished episodes: each shaped term's weighted sum per episode
                rec.update({k: v for k, v in envs.shaping_stats(reset=True).items() if k.startswith("sr/")})
            if termination:                           # this rank's finished episodes: the share each rule ended
                rec.update(envs.termination_stats(reset=True))
            if kl_args:                               # the last update's mini-batch steps: mean KL estimate and clip fraction, the rate last used
                dg = agent.last_diagnostics
                rec.update(approx_kl=dg["approx_kl"], clip_fraction=dg["clip_fraction"], lr=dg["lr"], kl_stopped_steps=dg["steps"] - dg["steps_applied"])
            history.append(rec)
            if rank == 0:
                print("Updates {update}, num timesteps {timesteps}, FPS {fps}\n mean reward {ep_reward:.2f} mean length "
                      "{ep_length:.0f} mean success {success:.2f}\n entropy {entropy:.2f} value loss {value_loss:.3f} "
                      "action loss {action_loss:.3f}".format(**rec), flush=True)
                if writer is not None:
                    for k in ("value_loss", "action_loss", "entropy", "ep_reward", "ep_length", "success"):
                        writer.add_scalar(k, rec[k], total)
                    for k in ("approx_kl", "clip_fraction", "lr", "kl_stopped_steps") if kl_args else ():
                        writer.add_scalar(k, rec[k], total)
                    for k in rec:
                        if k.startswith(("dr/", "sr/", "term/")):   # agents/ppo/train.py:98-100, utils.log of the dr/ deques; sr/: shaped terms; term/: early terminations
                            writer.add_scalar(k, rec[k], total)
    return actor_critic, history
