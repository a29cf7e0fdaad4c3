#!/usr/bin/env python3
"""Headless evaluation of a trained policy (the role of the reference's GUI script testing/test_ppo.py:17-151):
loads `<checkpoint-dir>/solo.pt` (same dict keys as the reference's checkpoint, agents/ppo/train.py:121-131),
rolls it out on the HIP engine until --num-runs episodes have ended and prints
`mean length / mean reward / mean success` (test_ppo.py:147).  In place of the GUI, --dump writes env 0's
trajectory (base pose, joint angles, action, reward, done) to an .npz.  --push-interval K --push-max-vel V kicks the base of every env
every K control steps with an xy velocity drawn uniformly from +-V m/s (robustness evaluation; SoloVecEnv.push)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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
    p.add_argument("--push-interval", type=int, default=0, help="kick every env's base velocity every K control steps (0 = never)")
    p.add_argument("--push-max-vel", type=float, default=0.0, help="a kick's x and y velocity change is uniform in +-V m/s")
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
    env = make_vec_envs(config, a.num_agents, None, device=dev, training=False, seed=a.seed, norm_obs=ob_rms is not None)
    env.ob_rms = ob_rms
    env.eval()
    policy = Policy(env.observation_space.shape, env.action_space, None, {"hidden_size": a.hidden_size}).to(dev)
    policy.load_state_dict(ckpt["state_dict"])
    policy.eval()
    torch.manual_seed(a.seed)

    ep_len, ep_R, ep_succ = [], [], []
    ret = torch.zeros(a.num_agents, device=dev)
    traj = dict(pos=[], quat=[], q=[], action=[], reward=[], done=[])
    obs = env.reset()
    push_gen, steps = None, 0
    if a.push_interval > 0:
        push_gen = torch.Generator(device=dev); push_gen.manual_seed(a.seed)
        dv = torch.zeros((a.num_agents, 3), device=dev)
    while len(ep_len) < a.num_runs:
        if push_gen is not None and steps > 0 and steps % a.push_interval == 0:
            dv[:, :2] = (torch.rand((a.num_agents, 2), device=dev, generator=push_gen) * 2 - 1) * a.push_max_vel
            env.push(dv)
            obs = env.normalize_obs(env.get_observation())          # the policy sees the kicked velocities
        steps += 1
        with torch.no_grad():
            _, action, _ = policy.act(obs, deterministic=a.deterministic)
        if a.dump:
            s = env.get_state(0)
            traj["pos"].append(list(s.pos)); traj["quat"].append(list(s.quat)); traj["q"].append(list(s.q))
            traj["action"].append(action[0].cpu().numpy())
        obs, reward, done, infos = env.step(action)
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
    print("episodes {} mean length {:.1f} mean reward {:.3f} mean success {:.2f}".format(
        n, sum(ep_len) / n, sum(ep_R) / n, sum(ep_succ) / n))
    if a.dump:
        np.savez(a.dump, **{k: np.asarray(v) for k, v in traj.items()})
        print("trajectory of env 0 ({} steps) -> {}".format(len(traj["reward"]), a.dump))
    env.close()
    return dict(episodes=n, mean_length=sum(ep_len) / n, mean_reward=sum(ep_R) / n, mean_success=sum(ep_succ) / n)


if __name__ == "__main__":
    main()
