#!/usr/bin/env python
"""End-to-end check that the simulator is a LEARNABLE environment: PPO on a robot_lab velocity task, all of it on the MI355X.

    collect: 24 x (actor + critic [rl_policy.hip] -> sample [rl_rollout.hip] -> env.step [rl_env.hip]) + GAE, ONE hipGraph launch
    update:  robot_lab_amd/ppo.py (torch autograd; rsl_rl's PPO.update with the reference's hyper-parameters, rsl_rl_ppo_cfg.py:10-37)
    push:    rl_mlp_set_weights (the inference kernels keep their buffers: the captured graph stays valid)

What the reference runs as `python scripts/reinforcement_learning/rsl_rl/train.py --task ... --headless` (train.py:177-224) with
rsl-rl-lib, which is not installable here.  A robot that learns to follow velocity commands within a few hundred iterations is
evidence that observations, actions, actuators, contacts, rewards, resets and curricula hang together - something no per-step
parity test against our own oracle can show.
`--learner hip` runs the update as HIP kernels instead (robot_lab_amd/ppo_hip.py, csrc/rl_ppo.hip) and pushes with rl_mlp_set_weights_device.
`--symmetry lr` (or `lr,fb`) turns on symmetry data augmentation inside the update of either learner (`Trainer(symmetry=...)`);
`--mirror-loss C` adds rsl_rl's mirror loss with coefficient C on the same tables, `--no-data-augmentation` keeps the mirror loss alone.
`--obs-normalization` normalises both observation groups; with `--normalize-in-learner` the learners read the raw storage and normalise for
themselves (`Trainer(normalize_in_learner=True)`), which is what `--symmetry` / `--mirror-loss` need together with it.
`--recurrent [--rnn-hidden-dim 256]` trains rsl_rl's `ActorCriticRecurrent` (an LSTM in front of 128-128-128 heads, the reference's recurrent agent cfgs):
the cells run in the captured collection (csrc/rl_lstm.hip), the update is robot_lab_amd/recurrent.py on torch or - `--recurrent-learner hip` - back-propagation
through time as HIP kernels (robot_lab_amd/recurrent_hip.py, csrc/learner/rl_bptt.inl), pushed into cells and heads device to device.
    python tools/train_demo.py [--task ID] [--num-envs N] [--iterations K] [--learner torch|hip] [--symmetry lr|fb|lr,fb] [--mirror-loss C]
                               [--no-data-augmentation] [--obs-normalization [--normalize-in-learner]] [--recurrent [--rnn-hidden-dim H] [--recurrent-learner torch|hip]] [--out DIR]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robot_lab_amd.env import ManagerBasedRLEnv  # noqa: E402
from robot_lab_amd.ppo import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--learner", choices=("torch", "hip"), default="torch", help="torch: autograd (robot_lab_amd/ppo.py); hip: the HIP learner (robot_lab_amd/ppo_hip.py)")
    ap.add_argument("--symmetry", default=None, help="mirrors of the symmetry data augmentation inside the update: lr, fb or lr,fb (default: none)")
    ap.add_argument("--mirror-loss", type=float, default=None, metavar="C", help="coefficient of the mirror loss on the --symmetry tables (default: off)")
    ap.add_argument("--no-data-augmentation", action="store_true", help="with --mirror-loss: the PPO terms stay on the stored rows")
    ap.add_argument("--obs-history", type=int, default=0, metavar="N", help="policy-group observation history of N frames (IsaacLab's ObservationGroupCfg.history_length)")
    ap.add_argument("--obs-normalization", action="store_true", help="rsl_rl's empirical normalisation of both observation groups (actor_obs_normalization, critic_obs_normalization)")
    ap.add_argument("--normalize-in-learner", action="store_true",
                    help="with --obs-normalization: the learners normalise the raw stored rows themselves (needed together with --symmetry / --mirror-loss)")
    ap.add_argument("--recurrent", action="store_true", help="an LSTM in front of 128-128-128 actor / critic heads (Trainer(rnn_type=\"lstm\")); its learner is --recurrent-learner, not --learner")
    ap.add_argument("--rnn-hidden-dim", type=int, default=256, metavar="H", help="with --recurrent: the LSTM's hidden width")
    ap.add_argument("--recurrent-learner", choices=("torch", "hip"), default="torch",
                    help="with --recurrent: torch autograd through time (robot_lab_amd/recurrent.py) or the HIP learner (robot_lab_amd/recurrent_hip.py)")
    ap.add_argument("--rnd-weight", type=float, default=None, metavar="W", help="random network distillation (Trainer(rnd=...)): weight of the intrinsic reward; "
                    "predictor and target 256-256 -> 1 on the policy group")
    ap.add_argument("--rnd-reward-normalization", action="store_true", help="with --rnd-weight: the intrinsic reward over the running std of its discounted average")
    ap.add_argument("--rnd-state-normalization", action="store_true", help="with --rnd-weight: empirical normalisation of the RND state")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpurun_out"))
    ap.add_argument("--print-every", type=int, default=10)
    ap.add_argument("--save", default=None, metavar="PATH", help="also write a checkpoint in the runner's layout (model_state_dict / optimizer_state_dict / iter / infos): "
                    "what tools/distill_demo.py --teacher and the runners' load() read")
    ap.add_argument("--also-terminate-on", default="", help="DIAGNOSTIC, not the reference's cfg: regex of body names added to the illegal-contact termination")
    a = ap.parse_args()
    if not a.symmetry and (a.mirror_loss is not None or a.no_data_augmentation):
        ap.error("--mirror-loss / --no-data-augmentation need --symmetry")
    if a.normalize_in_learner and not a.obs_normalization:
        ap.error("--normalize-in-learner needs --obs-normalization")
    if a.recurrent_learner != "torch" and not a.recurrent:
        ap.error("--recurrent-learner needs --recurrent")
    if a.rnd_weight is None and (a.rnd_reward_normalization or a.rnd_state_normalization):
        ap.error("--rnd-reward-normalization / --rnd-state-normalization need --rnd-weight")
    hist = {"policy": a.obs_history} if a.obs_history else None
    if a.also_terminate_on:
        import re

        from robot_lab_amd.scene import load_bundle

        desc, extra = load_bundle(a.task)
        hit = [i for i, n in enumerate(desc.body_names) if re.fullmatch(a.also_terminate_on, n)]
        for i in hit:
            desc.task.illegal_body_mask |= 1 << i
        desc.task.term_illegal_contact = 1
        print(f"DIAGNOSTIC run: illegal-contact termination extended to {[desc.body_names[i] for i in hit]}")
        env = ManagerBasedRLEnv(desc=desc, extra=extra, num_envs=a.num_envs, seed=a.seed, device="cuda:0", obs_history=hist)
    else:
        env = ManagerBasedRLEnv(a.task, num_envs=a.num_envs, seed=a.seed, device="cuda:0", obs_history=hist)
    print(env, flush=True)  # (names the step kernel: specialised on the task, or the interpreter)
    mirror = dict(mirror_loss=a.mirror_loss, data_augmentation=not a.no_data_augmentation) if a.symmetry else {}
    norm = dict(actor_obs_normalization=True, critic_obs_normalization=True, normalize_in_learner=a.normalize_in_learner) if a.obs_normalization else {}
    rnn = dict(rnn_type="lstm", rnn_hidden_dim=a.rnn_hidden_dim, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128), recurrent_learner=a.recurrent_learner) if a.recurrent else {}
    device_learner = a.learner == "hip" or (a.recurrent and a.recurrent_learner == "hip")  # the std the sampler reads and Adam's state live in the learner
    rnd = dict(rnd=dict(weight=a.rnd_weight, reward_normalization=a.rnd_reward_normalization, state_normalization=a.rnd_state_normalization,
                        predictor_hidden_dims=[256, 256], target_hidden_dims=[256, 256])) if a.rnd_weight is not None else {}
    tr = Trainer(env, seed=a.seed, learner=a.learner, symmetry=a.symmetry, **mirror, **norm, **rnn, **rnd)
    print(tr, flush=True)
    # init_at_random_ep_len=True (train.py:224): the first time-outs are spread over an episode length
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (a.num_envs,), generator=torch.Generator().manual_seed(a.seed))
    names = list(env.desc.reward_names)
    track = [n for n in names if n.startswith("track_lin_vel_xy")][0]
    log, t_collect, t_update = [], 0.0, 0.0
    t_start = time.perf_counter()
    for it in range(a.iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.collector.collect()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        st = tr.storage
        row = dict(iteration=it, mean_step_reward=float(st.rewards.mean()), done_rate=float(st.dones.float().mean()))
        if tr.rnd_device is not None:
            intrinsic, total = tr.rnd_device.reward.sums()
            row.update(mean_intrinsic_reward=intrinsic / st.rewards.numel(), mean_extrinsic_reward=(total - intrinsic) / st.rewards.numel(), rnd_weight=tr.rnd_device.last_weight)
        row.update(tr.alg.update(tr.update_batch(), tr.gen))
        tr.push_parameters()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_collect += t1 - t0
        t_update += t2 - t1
        ex = env.extras.get("log", {})
        for k in ("Episode_Reward/" + track, "Metrics/base_velocity/error_vel_xy", "Metrics/base_velocity/error_vel_yaw", "Episode_Termination/time_out",
                  "Curriculum/terrain_levels"):
            if k in ex:
                row[k] = float(ex[k])
        row["action_std"] = float((tr.std if device_learner else tr.policy.std.detach()).mean())
        if it % a.print_every == 0 or it == a.iterations - 1:  # posture of the batch (an export of the state: only when a line is printed)
            d = env.scene["robot"].data
            qw = d.root_quat_w
            row["root_height"] = float((d.root_pos_w[:, 2] - env.scene.env_origins[:, 2]).mean())
            row["upright"] = float((1.0 - 2.0 * (qw[:, 1] ** 2 + qw[:, 2] ** 2)).mean())  # z component of the body's up axis: 1 = upright, 0 = on a side
        log.append(row)
        if it % a.print_every == 0 or it == a.iterations - 1:
            print(f"it {it:4d}  reward/step {row['mean_step_reward']:+.4f}  {track} {row.get('Episode_Reward/' + track, float('nan')):.3f}  "
                  f"err_xy {row.get('Metrics/base_velocity/error_vel_xy', float('nan')):.3f}  done/step {row['done_rate']:.4f}  std {row['action_std']:.3f}  "
                  f"lr {row['learning_rate']:.1e}  kl {row['kl']:.4f}  v_loss {row['value_loss']:.4f}  "
                  + (f"rnd_loss {row['rnd_loss']:.3e}  r_int {row['mean_intrinsic_reward']:+.4f}  r_ext {row['mean_extrinsic_reward']:+.4f}  " if "rnd_loss" in row else "") +
                  f"height {row.get('root_height', float('nan')):.3f}  upright {row.get('upright', float('nan')):+.3f}", flush=True)
    wall = time.perf_counter() - t_start
    n_steps = a.iterations * st.num_transitions_per_env * a.num_envs
    summary = dict(task=a.task, learner=a.learner, recurrent=bool(a.recurrent), recurrent_learner=a.recurrent_learner if a.recurrent else None, rnn_hidden_dim=a.rnn_hidden_dim if a.recurrent else None, symmetry=a.symmetry, mirror_loss=a.mirror_loss, data_augmentation=not a.no_data_augmentation, step_kernel=env.step_kernel, obs_history=env.obs_history, obs_normalization=bool(a.obs_normalization), rnd=rnd.get("rnd"), normalize_in_learner=bool(a.normalize_in_learner), num_envs=a.num_envs, iterations=a.iterations, wall_s=wall, env_steps=n_steps, env_steps_per_s=n_steps / wall,
                   collect_ms_per_iteration=1e3 * t_collect / a.iterations, update_ms_per_iteration=1e3 * t_update / a.iterations,
                   first=log[0], last=log[-1])
    print(json.dumps({k: v for k, v in summary.items() if k not in ("first", "last")}))
    os.makedirs(a.out, exist_ok=True)
    tag = a.task.replace("RobotLab-Isaac-Velocity-", "").replace("-v0", "") + ("_recurrent" if a.recurrent else "") + ("_hip" if a.recurrent and a.recurrent_learner == "hip" else "") + ("_rnd" if rnd else "")
    with open(os.path.join(a.out, f"train_demo_{tag}.json"), "w") as f:
        json.dump(dict(summary=summary, log=log), f, indent=1)
    torch.save(tr.state_dict(), os.path.join(a.out, f"train_demo_{tag}.pt"))
    if a.save:
        optimizer_state = tr.alg.optimizer_state_dict() if device_learner else tr.alg.optimizer.state_dict()
        os.makedirs(os.path.dirname(os.path.abspath(a.save)), exist_ok=True)
        torch.save({"model_state_dict": tr.state_dict(), "optimizer_state_dict": optimizer_state, "iter": a.iterations, "infos": None}, a.save)
        print(f"checkpoint in the runner's layout: {a.save}")
    env.close()


if __name__ == "__main__":
    main()
