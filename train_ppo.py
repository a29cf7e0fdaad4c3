#!/usr/bin/env python3
"""Launcher with the reference's flag names (training/train_ppo.py:9-45) and YAML task definitions
(configs/*.yaml).  Single GPU:  python train_ppo.py --config-file configs/basic12.yaml --task walk
--num-agents 4096 --use-gae --use-linear-lr-decay ...   Multi GPU (one process per GPU, RCCL):
python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train_ppo.py ..."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def push_interval(text):
    """--push-interval LO[:HI] -> (lo, hi): control steps between two kicks of an env, 1 <= lo <= hi"""
    try:
        parts = [int(x) for x in text.split(":")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2) or parts[0] < 1 or parts[-1] < parts[0]:
        raise argparse.ArgumentTypeError("expected LO or LO:HI with 1 <= LO <= HI, got %r" % text)
    return parts[0], parts[-1]


def action_delay(text):
    """--action-delay LO[:HI] -> (lo, hi): control steps of actuation latency, 0 <= lo <= hi <= 4"""
    try:
        parts = [int(x) for x in text.split(":")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2) or parts[0] < 0 or parts[-1] < parts[0] or parts[-1] > 4:
        raise argparse.ArgumentTypeError("expected LO or LO:HI with 0 <= LO <= HI <= 4, got %r" % text)
    return parts[0], parts[-1]


def motor_gain_range(text):
    """--motor-gain-range G -> G, 0 <= G < 1"""
    try:
        g = float(text)
    except ValueError:
        g = -1.0
    if not 0.0 <= g < 1.0:
        raise argparse.ArgumentTypeError("expected a gain range in [0, 1), got %r" % text)
    return g


def add_channel_flags(p):
    """the flags train_ppo.py and eval_ppo.py share"""
    p.add_argument("--commands", type=str, default=None, metavar="FILE.yaml",
                   help="per-env velocity commands: ranges of lin_vel_x, lin_vel_y and yaw_rate, `interval`, `zero_prob`, `min_lin_norm`, "
                        "`obs_scale`, e.g. configs/commands_walk12.yaml; the observation gains three words and the tracking terms of "
                        "--reward-shaping follow each env's own command (default: no commands)")
    p.add_argument("--termination", type=str, default=None, metavar="FILE.yaml",
                   help="early termination rules checked on the state after every step: `base_height`, `max_tilt_deg`, `contacts` with "
                        "`contact_force_min`, `joint_limits`, `min_steps`, `terminal_reward`, e.g. configs/termination_walk12.yaml (default: "
                        "the engine's own endings only)")
    p.add_argument("--reset-randomization", type=str, default=None, metavar="FILE.yaml",
                   help="randomised initial states behind every reset: half-widths `joint_pos`, `joint_vel`, `lin_vel`, `ang_vel`, `yaw`, "
                        "`roll`, `pitch`, and `place_on_ground` with `clearance`, e.g. configs/reset_walk12.yaml (default: the engine's own "
                        "snapshots)")
    p.add_argument("--obs-noise", type=str, default=None, metavar="FILE.yaml",
                   help="uniform sensor noise on every observation: `groups:` (observation group -> half-width in physical units) and "
                        "`history:`, e.g. configs/noise_solo.yaml (default: clean observations)")
    p.add_argument("--action-delay", type=action_delay, default=None, metavar="LO[:HI]",
                   help="every env applies the action it received LO..HI control steps ago (drawn per env and episode, at most 4; default: none)")
    p.add_argument("--motor-gain-range", type=motor_gain_range, default=0.0, metavar="G",
                   help="each joint's action is scaled by 1 + U(-G, G), drawn per env and episode (default: 0, exact)")


def load_option(flag, path, validate):
    """--flag FILE.yaml -> validate(the file's dict), with unknown keys and bad values refused by name before anything is built"""
    from solorl_amd.config import load_yaml
    try:
        return validate(load_yaml(path))
    except (ValueError, AttributeError, TypeError) as e:
        raise SystemExit("%s %s: %s" % (flag, path, e))


def _checked(check):
    """validate for load_option: the file's dict itself, once ``check`` has taken it"""
    def validate(d):
        check(d)
        return d
    return validate


def load_reward_shaping(path):
    from solorl_amd.shaping import params_from_dict
    return load_option("--reward-shaping", path, _checked(params_from_dict))


def load_obs_noise(path, config):
    from solorl_amd.channel import scales_from_dict
    from solorl_amd.config import config_from_dict
    return load_option("--obs-noise", path, _checked(lambda d: scales_from_dict(config_from_dict(config), d)))


def load_commands(path):
    from solorl_amd.command import ranges_from_dict
    return load_option("--commands", path, ranges_from_dict)


def load_termination(path, config):
    from solorl_amd.config import config_from_dict
    from solorl_amd.termination import make_termination, rules_from_dict
    return load_option("--termination", path, _checked(lambda d: make_termination(config_from_dict(config), **rules_from_dict(d))))


def load_reset_randomization(path, config):
    from solorl_amd.config import config_from_dict
    from solorl_amd.reset_random import make_reset_randomization, ranges_from_dict
    return load_option("--reset-randomization", path,
                       _checked(lambda d: make_reset_randomization(config_from_dict(config), 0, 0, **ranges_from_dict(d))))


def load_privileged_critic(path, config):
    from solorl_amd.config import config_from_dict
    from solorl_amd.critic_obs import make_params, scales_from_dict
    return load_option("--privileged-critic", path, _checked(lambda d: make_params(config_from_dict(config), 1, **scales_from_dict(d))))


def get_ppo_args(argv=None):
    p = argparse.ArgumentParser("PPO args")
    p.add_argument("--num-agents", type=int, default=32)          # envs PER GPU
    p.add_argument("--output-size", type=int, default=64)         # accepted and unused, as in the reference (train_ppo.py:12)
    p.add_argument("--hidden-size", type=int, default=64)
    p.add_argument("--no-cuda", action="store_true", default=False)
    p.add_argument("--no-hip-graphs", action="store_true", default=False, help="run rollout and update eagerly instead of replaying HIP graphs")
    p.add_argument("--env-name", type=str, default="base")
    p.add_argument("--gamma", type=float, default=0.99)
    p.add_argument("--tau", type=float, default=0.95)
    p.add_argument("--clip-param", type=float, default=0.1)
    p.add_argument("--ppo-epoch", type=int, default=10)
    p.add_argument("--mini-batch-size", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--l2-coef", type=float, default=0.0)
    p.add_argument("--value-loss-coef", type=float, default=0.5)
    p.add_argument("--entropy-coef", type=float, default=0.01)
    p.add_argument("--max-grad-norm", type=float, default=0.5)
    p.add_argument("--clip-value-loss", action="store_true", default=False)   # accepted; the reference's PPO always clips the value
                                                                               # loss (ppo.py:18 default, the flag is never forwarded)
    p.add_argument("--use-linear-lr-decay", action="store_true", default=False)
    p.add_argument("--use-gae", action="store_true", default=False)
    p.add_argument("--num-env-steps", type=float, default=1e6)
    p.add_argument("--seed", type=int, default=2301)
    p.add_argument("--curriculum-schedule", type=int, default=0)
    p.add_argument("--log-interval", type=int, default=10)
    p.add_argument("--logdir", type=str, default=None)
    p.add_argument("--base-checkpoint", type=str, default=None)
    p.add_argument("--timestamp", type=str, default=None)
    p.add_argument("--save-interval", type=int, default=20)
    p.add_argument("--config-file", type=str, default="configs/basic.yaml")
    p.add_argument("--task", type=str, default=None)
    p.add_argument("--normalize-obs", action="store_true", default=False, help="running observation normalisation (VecNormalize ob=True)")
    p.add_argument("--normalize-returns", action="store_true", default=False, help="running return normalisation of the rewards (VecNormalize ret=True, discount --gamma)")
    p.add_argument("--push-interval", type=push_interval, default=None, metavar="LO[:HI]",
                   help="kick every training env's base every LO..HI control steps (drawn on the device; default: no kicks)")
    p.add_argument("--push-max-vel", type=float, default=0.0, help="a kick adds U(-V, V) m/s to the base's world x and y velocity")
    p.add_argument("--push-max-yaw-rate", type=float, default=0.0, help="... and U(-W, W) rad/s to its yaw rate")
    p.add_argument("--reward-shaping", type=str, default=None, metavar="FILE.yaml",
                   help="add shaped reward terms to every step's reward: `weights:` (term name -> weight) and the terms' parameters, "
                        "e.g. configs/shaping_walk12.yaml (default: the reference's reward alone)")
    add_channel_flags(p)
    p.add_argument("--privileged-critic", type=str, nargs="?", const=True, default=None, metavar="FILE.yaml",
                   help="asymmetric actor-critic: the value function reads rows of its own -- the observation before --obs-noise plus twenty "
                        "words of the simulator's truth (contact forces, foot heights and speeds, the command, the episode's progress, "
                        "collisions, the drawn latency and gain error, the last kick); FILE.yaml holds scales per group of words, e.g. "
                        "configs/critic_walk12.yaml (without a file: the defaults; default: the critic reads the actor's rows)")
    p.add_argument("--bootstrap-timeouts", action="store_true", default=False,
                   help="time-limit bootstrapping: a step the time limit cut off bootstraps its return from the value of the observation its "
                        "action was taken from, instead of reading as a fall (default: off, the reference's returns)")
    p.add_argument("--generic-policy-kernels", action="store_true", default=False,
                   help="run a policy shape the per-shape policy kernels are not built for (e.g. --commands with a history level: 79 wide) on "
                        "the width-generic kernels instead of the PyTorch path: any observation and critic width up to 128 "
                        "(sets SOLORL_POLICY_GENERIC=1; default: off)")
    p.add_argument("--desired-kl", type=float, default=None, metavar="D",
                   help="adaptive learning rate: after every mini-batch step's KL estimate, lr / 1.5 above 2 D and lr * 1.5 below D / 2, within "
                        "[1e-5, 1e-2] (rsl_rl's schedule, decided on the device; not with --use-linear-lr-decay; default: off)")
    p.add_argument("--target-kl", type=float, default=None, metavar="K",
                   help="end an update's mini-batch steps once the KL estimate exceeds 1.5 K (stable-baselines' target_kl; default: off)")
    p.add_argument("--ppo-diagnostics", action="store_true", default=False,
                   help="log approx_kl, clip_fraction and lr of every update (on by itself with --desired-kl / --target-kl; default: off)")
    p.add_argument("--num-steps", type=int, default=None, help="rollout length (default: episode_length, train_ppo.py:62-63)")
    return p.parse_args(argv)


def main(argv=None):
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    args = get_ppo_args(argv)
    config = load_yaml(args.config_file)
    if args.task is not None:
        config["task"] = args.task      # the override the reference left commented out (train_ppo.py:57-60)
    if args.env_name != "base":
        raise SystemExit("--env-name %s needs the absent `scripts.Controller` (SURVEY.md section 0.6); only 'base' is provided" % args.env_name)
    args.cuda = not args.no_cuda
    if args.generic_policy_kernels:
        os.environ["SOLORL_POLICY_GENERIC"] = "1"       # read by ppo/graphs.py when the loops are built
    if not args.cuda:
        raise SystemExit("the rollout engine is GPU-only (no CPU fallback)")
    if args.num_steps is None:
        args.num_steps = config["episode_length"]
    if args.reward_shaping is not None:
        args.reward_shaping = load_reward_shaping(args.reward_shaping)
    if args.obs_noise is not None:
        args.obs_noise = load_obs_noise(args.obs_noise, config)
    if args.commands is not None:
        args.commands = load_commands(args.commands)
    if args.termination is not None:
        args.termination = load_termination(args.termination, config)
    if args.reset_randomization is not None:
        args.reset_randomization = load_reset_randomization(args.reset_randomization, config)
    if args.privileged_critic is not None:
        if args.normalize_obs:
            raise SystemExit("--privileged-critic with --normalize-obs: the critic rows would need running statistics of their own")
        if args.privileged_critic is not True:
            args.privileged_critic = load_privileged_critic(args.privileged_critic, config)
    writer = None
    rank = int(os.environ.get("RANK", "0"))
    if args.logdir is not None:      # run directory named as training/train_ppo.py:64-72
        from datetime import datetime
        # under torch.distributed.run every rank runs main(): the stamp comes from the launcher's start time when it exports one
        # (TORCHELASTIC_RUN_ID does not carry it), else from this rank's clock -- only rank 0's directory is ever written to
        stamp = datetime.now().strftime("%Y%m%d-%H%M%S") if args.timestamp is None else datetime.now().strftime("%Y%m%d-") + args.timestamp
        task = args.task + "_" if args.task is not None else ""
        args.logdir = os.path.join(args.logdir, "Solo" + args.env_name.capitalize() + "_" + task + stamp)
        if rank == 0:                # the reference is single-process; with N ranks only rank 0 logs and saves
            try:                     # tensorboard is optional here (not installed in the build image)
                from torch.utils.tensorboard import SummaryWriter
                writer = SummaryWriter(args.logdir)
            except Exception:
                writer = None
    return train(args, config, None, writer)


if __name__ == "__main__":
    main()
