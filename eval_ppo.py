#!/usr/bin/env python3
"""Headless evaluation of a trained policy (the role of the reference's GUI script testing/test_ppo.py:17-151):
loads `<checkpoint-dir>/solo.pt` (same dict keys as the reference's checkpoint, agents/ppo/train.py:121-131),
rolls it out on the HIP engine until --num-runs episodes have ended and prints
`mean length / mean reward / mean success` (test_ppo.py:147).  In place of the GUI, --dump writes env 0's
trajectory (base pose, joint angles, action, reward, done) to an .npz.  --push-interval K --push-max-vel V kicks the base of every env
every K control steps with an xy velocity drawn uniformly from +-V m/s (robustness evaluation; SoloVecEnv.push).
--gait-metrics says what the gait looks like, from the batched kinematics of every env at every step (SoloVecEnv.get_kinematics,
reduced on the device): per foot the duty factor, mean and peak normal force, slip distance and peak swing clearance, and the mean
ratio of the summed normal forces to the robot's weight; --dump then also holds env 0's foot positions and forces.
--obs-noise FILE.yaml --action-delay LO[:HI] --motor-gain-range G (train_ppo.py's flags) evaluate under sensor noise, actuation latency
and motor gain error (SoloVecEnv.set_obs_noise / set_actuation).
--commands FILE.yaml (train_ppo.py's flag) evaluates a policy trained with per-env velocity commands under commands drawn from the file's
ranges; --command VX VY WZ gives every env that one command for the whole run (joystick control).  With either, the summary adds the
mean absolute tracking error of the base-frame velocity xy [m/s] and of the base-frame yaw rate [rad/s] over all envs and steps.
--termination FILE.yaml (train_ppo.py's flag) evaluates under early termination rules (SoloVecEnv.set_termination); the summary adds the
share of the finished episodes that each rule ended.
--reset-randomization FILE.yaml (train_ppo.py's flag) evaluates from randomised initial states (SoloVecEnv.set_reset_randomization)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


FEET = ("FL", "FR", "HL", "HR")


class GaitMetrics:
    """Per-foot sums over envs and steps, kept on the device; one transfer in report()."""

    def __init__(self, env):
        import torch
        self.dt = env.cfg.frame_skip * env.cfg.sim_dt            # control step [s]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=env.device)
        self.steps, self.contact, self.force, self.slip = 0, z(4), z(4), z(env.nenvs, 4)
        self.peak_force, self.clearance, self.support = z(4), z(4), z()

    def add(self, env, states, kin):
        """states: the StateBatch of SoloVecEnv.get_states(); kin: the KinBatch computed from it"""
        import torch
        from solorl_amd.kinematics import FOOT_PRIMS
        bits = torch.tensor(FOOT_PRIMS, device=env.device, dtype=torch.int32)
        touch = ((states.contact_mask.unsqueeze(1) >> bits) & 1).bool()          # [N, 4]
        self.steps += 1
        self.contact += touch.sum(0)
        self.force += kin.foot_force.sum(0)
        self.peak_force = torch.maximum(self.peak_force, kin.foot_force.max(0).values)
        self.slip += torch.where(touch, kin.foot_vel[:, :, :2].norm(dim=2) * self.dt, 0.0)
        self.clearance = torch.maximum(self.clearance, torch.where(touch, 0.0, kin.foot_pos[:, :, 2]).max(0).values)
        self.support += (kin.prim_force.sum(1) / (kin.mass * env.cfg.gravity)).mean()

    def report(self):
        n = self.slip.shape[0] * max(self.steps, 1)
        out = dict(steps=self.steps, support_ratio=float(self.support) / max(self.steps, 1),
                   duty_factor=(self.contact / n).tolist(), mean_force=(self.force / n).tolist(), peak_force=self.peak_force.tolist(),
                   slip_distance=self.slip.mean(0).tolist(), peak_clearance=self.clearance.tolist())
        print("gait over {} steps: mean sum of normal forces / weight {:.3f}".format(self.steps, out["support_ratio"]))
        for f, name in enumerate(FEET):
            print("  {} duty factor {:.3f}  normal force mean {:.2f} N peak {:.2f} N  slip {:.4f} m  peak swing clearance {:.4f} m".format(
                name, out["duty_factor"][f], out["mean_force"][f], out["peak_force"][f], out["slip_distance"][f], out["peak_clearance"][f]))
        return out


def base_frame(quat, v):
    """R(quat)^T v for rows of unit quaternions (x, y, z, w) and world-frame vectors [N, 3]: v - 2 w (u x v) + 2 u x (u x v), u = quat.xyz"""
    import torch
    u, w = quat[:, :3], quat[:, 3:4]
    c = torch.cross(u, v, dim=1)
    return v - 2.0 * w * c + 2.0 * torch.cross(u, c, dim=1)


def main(argv=None):
    p = argparse.ArgumentParser("PPO eval")
    p.add_argument("--checkpoint-dir", required=True)
    p.add_argument("--config-file", default="configs/basic.yaml")
    p.add_argument("--task", default=None)
    p.add_argument("--num-runs", type=int, default=10)
    p.add_argument("--num-agents", type=int, default=64)
    p.add_argument("--hidden-size", type=int, default=64)
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--dump", default=None, help="write env 0's trajectory to this .npz")
    p.add_argument("--gait-metrics", action="store_true", help="per-foot duty factor, normal force, slip and swing clearance over all envs and steps")
    p.add_argument("--max-steps", type=int, default=0, help="stop after K control steps even if fewer than --num-runs episodes have ended (0 = no limit)")
    p.add_argument("--push-interval", type=int, default=0, help="kick every env's base velocity every K control steps (0 = never)")
    p.add_argument("--push-max-vel", type=float, default=0.0, help="a kick's x and y velocity change is uniform in +-V m/s")
    from train_ppo import add_channel_flags, load_commands, load_obs_noise, load_reset_randomization, load_termination
    add_channel_flags(p)
    p.add_argument("--command", type=float, nargs=3, default=None, metavar=("VX", "VY", "WZ"),
                   help="one fixed velocity command for every env: vx vy [m/s, base frame] and yaw rate [rad/s]; with --commands it keeps "
                        "the file's obs_scale and replaces its ranges")
    a = p.parse_args(argv)

    import numpy as np
    import torch
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import make_vec_envs

    config = load_yaml(a.config_file)
    if a.task is not None:
        config["task"] = a.task
    ckpt = torch.load(os.path.join(a.checkpoint_dir, "solo.pt"), map_location="cpu", weights_only=False)
    dev = torch.device("cuda:0")
    # a checkpoint trained with --normalize-obs carries the observation statistics: the policy sees observations scaled by them,
    # frozen (testing/test_ppo.py:89-90); rewards are reported raw
    ob_rms = ckpt.get("ob_rms")
    commands = None if a.commands is None else load_commands(a.commands)
    if a.command is not None:           # lo == hi, redrawn at every step, never zeroed: every env holds exactly this command
        vx, vy, wz = a.command
        commands = dict(obs_scale=(commands or {}).get("obs_scale", (1.0, 1.0, 1.0)), lin_vel_x=(vx, vx), lin_vel_y=(vy, vy), yaw_rate=(wz, wz),
                        interval=1, zero_prob=0.0, min_lin_norm=0.0)
    env = make_vec_envs(config, a.num_agents, None, device=dev, training=False, seed=a.seed, norm_obs=ob_rms is not None,
                        obs_noise=None if a.obs_noise is None else load_obs_noise(a.obs_noise, config), action_delay=a.action_delay,
                        motor_gain_range=a.motor_gain_range, commands=commands,
                        termination=None if a.termination is None else load_termination(a.termination, config),
                        reset_randomization=None if a.reset_randomization is None else load_reset_randomization(a.reset_randomization, config))
    width = ckpt["state_dict"]["base.features.0.weight"].shape[1]
    if width != env.obs_dim:
        raise SystemExit("the checkpoint's policy reads %d observation words, this run's observation has %d (%d of the engine%s): "
                         "a policy trained %s --commands needs them %s" % (
                             width, env.obs_dim, env.engine_obs_dim, " + 3 command words" if commands is not None else "",
                             "with" if width == env.engine_obs_dim + 3 else "without", "given here" if commands is None else "left out"))
    env.ob_rms = ob_rms
    env.eval()
    # a checkpoint trained with --privileged-critic: its critic reads rows of another width (the names are the same).  Evaluation runs
    # the actor alone, which needs no critic rows: the env is made without them
    critic_width = ckpt["state_dict"]["base.critic.0.weight"].shape[1]
    policy = Policy(env.observation_space.shape, env.action_space, None, {"hidden_size": a.hidden_size},
                    critic_obs_dim=None if critic_width == width else critic_width).to(dev)
    policy.load_state_dict(ckpt["state_dict"])
    policy.eval()
    torch.manual_seed(a.seed)

    ep_len, ep_R, ep_succ = [], [], []
    ret = torch.zeros(a.num_agents, device=dev)
    traj = dict(pos=[], quat=[], q=[], action=[], reward=[], done=[], foot_pos=[], foot_force=[])
    gait = GaitMetrics(env) if a.gait_metrics else None
    rows = kin = None
    obs = env.reset()
    push_gen, steps = None, 0
    track = torch.zeros(2, dtype=torch.float64, device=dev) if commands is not None else None     # sums of |v_b.xy - cmd.xy| and |w_b.z - cmd.z|
    track_rows, track_n = None, 0.0
    if a.push_interval > 0:
        push_gen = torch.Generator(device=dev); push_gen.manual_seed(a.seed)
        dv = torch.zeros((a.num_agents, 3), device=dev)
    while len(ep_len) < a.num_runs and not (a.max_steps and steps >= a.max_steps):
        if push_gen is not None and steps > 0 and steps % a.push_interval == 0:
            dv[:, :2] = (torch.rand((a.num_agents, 2), device=dev, generator=push_gen) * 2 - 1) * a.push_max_vel
            env.push(dv)
            obs = env.normalize_obs(env.get_observation())          # the policy sees the kicked velocities
        steps += 1
        with torch.no_grad():
            if policy.critic_obs_dim is None:
                _, action, _ = policy.act(obs, deterministic=a.deterministic)
            else:                                        # an asymmetric checkpoint: the actor alone (there are no critic rows here)
                action = policy.act_actor(obs, deterministic=a.deterministic)
        if gait is not None or a.dump:
            rows = env.get_states(out=rows)              # the state the policy has just seen, every env: two launches
            kin = env.get_kinematics(states=rows, out=kin)
            if gait is not None:
                gait.add(env, rows, kin)
        if a.dump:
            traj["foot_pos"].append(kin.foot_pos[0].cpu().numpy()); traj["foot_force"].append(kin.foot_force[0].cpu().numpy())
            s = env.get_state(0)
            traj["pos"].append(list(s.pos)); traj["quat"].append(list(s.quat)); traj["q"].append(list(s.q))
            traj["action"].append(action[0].cpu().numpy())
        if track is not None:
            cmd = env.last_commands.clone()              # the command the policy has just acted on (the step may redraw it)
        obs, reward, done, infos = env.step(action)
        if track is not None:                            # the state after the step against that command; an env the step finished holds
            track_rows = env.get_states(out=track_rows)  # its reset state and is left out
            vb, wb = base_frame(track_rows.quat, track_rows.lin_vel), base_frame(track_rows.quat, track_rows.ang_vel)
            live = (done == 0).to(torch.float64)
            track[0] += ((vb[:, :2] - cmd[:, :2]).norm(dim=1) * live).sum()
            track[1] += ((wb[:, 2] - cmd[:, 2]).abs() * live).sum()
            track_n += float(live.sum())
        ret += reward.view(-1)
        if a.dump:
            traj["reward"].append(float(reward[0])); traj["done"].append(float(done[0]))
        idx = torch.nonzero(done).view(-1).tolist()
        if idx:
            T = infos.tensors
            for i in idx:
                ep_len.append(int(T["episode_length"][i])); ep_succ.append(float(T["success"][i])); ep_R.append(float(ret[i]))
            ret[done.bool()] = 0
    n = len(ep_len)
    mean = lambda v: sum(v) / n if n else float("nan")      # (--max-steps can end the run before any episode has)
    print("episodes {} mean length {:.1f} mean reward {:.3f} mean success {:.2f}".format(n, mean(ep_len), mean(ep_R), mean(ep_succ)))
    result = dict(episodes=n, mean_length=mean(ep_len), mean_reward=mean(ep_R), mean_success=mean(ep_succ))
    if track is not None:
        e = (track / max(track_n, 1.0)).tolist()
        print("command tracking over {:.0f} env steps: mean |v_b.xy - cmd.xy| {:.4f} m/s  mean |w_b.z - cmd.z| {:.4f} rad/s".format(track_n, e[0], e[1]))
        result["tracking_error_lin_vel"], result["tracking_error_yaw_rate"] = e
    if a.termination is not None:
        ts = env.termination_stats()
        print("early termination over {} finished episodes: {}".format(ts["term/episodes"], "  ".join(
            "{} {:.3f}".format(k[5:], v) for k, v in ts.items() if k != "term/episodes")))
        result["termination"] = ts
    if gait is not None:
        result["gait"] = gait.report()
    if a.dump:
        np.savez(a.dump, **{k: np.asarray(v) for k, v in traj.items()})
        print("trajectory of env 0 ({} steps) -> {}".format(len(traj["reward"]), a.dump))
    env.close()
    return result


if __name__ == "__main__":
    main()
