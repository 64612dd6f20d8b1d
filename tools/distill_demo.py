#!/usr/bin/env python
"""Distil a trained teacher into a small student, all of it on the MI355X: the second half of rsl_rl's "train a teacher with PPO, then
distil it" recipe (the reference's `train.py --agent=rsl_rl_distillation_cfg_entry_point --load_run <teacher>`).

    collect: 120 x (student + teacher in one launch [rl_policy.hip] -> sample [rl_rollout.hip] -> env.step [rl_env.hip]), ONE hipGraph launch
    update:  robot_lab_amd/distill.py (torch autograd; rsl_rl's Distillation.update) or, --learner hip, robot_lab_amd/distill_hip.py
    push:    the student into its inference kernel in place

A1 Flat with the numbers of the reference's rsl_rl_distillation_cfg.py: student 128-128-128, 120 steps per env, gradient length 15, two epochs,
learning rate 1e-3, init_std 0.1.  The teacher is a checkpoint in the runner's layout, e.g. of `tools/train_demo.py --save teacher.pt`
(its actor becomes the teacher; the teacher's hidden widths are read from it).
`--recurrent`: a recurrent student (an LSTM of 256 in front of the 128-128-128 MLP, robot_lab_amd/distill_recurrent.py) and the teacher of a
recurrent PPO checkpoint (`tools/train_demo.py --recurrent --save teacher.pt`: its memory_a and actor); `--mlp-teacher`: a feed-forward teacher's
checkpoint distilled into the recurrent student.
    python tools/distill_demo.py --teacher model.pt [--recurrent [--mlp-teacher]] [--learner torch|hip] [--iterations n] [--num-envs N] [--save PATH]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robot_lab_amd.distill import DistillTrainer  # noqa: E402
from robot_lab_amd.env import ManagerBasedRLEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--teacher", required=True, help="a PPO checkpoint in the runner's layout (model_state_dict with actor.* keys)")
    ap.add_argument("--task", default="RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--learner", choices=("torch", "hip"), default="torch")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--save", default=None, metavar="PATH", help="write the distilled policy as a checkpoint in the runner's layout")
    ap.add_argument("--recurrent", action="store_true", help="a recurrent student; the teacher is a recurrent PPO checkpoint unless --mlp-teacher")
    ap.add_argument("--mlp-teacher", action="store_true", help="with --recurrent: the teacher is a feed-forward PPO checkpoint")
    a = ap.parse_args()
    if a.mlp_teacher and not a.recurrent:
        ap.error("--mlp-teacher goes with --recurrent")
    d = torch.load(a.teacher, map_location="cpu", weights_only=False)
    sd = d["model_state_dict"] if "model_state_dict" in d else d
    net = "actor" if any(k.startswith("actor.") for k in sd) else "teacher"  # (a distillation checkpoint resumes)
    layers = sorted(int(k.split(".")[1]) for k in sd if k.startswith(net + ".") and k.endswith(".weight"))
    if not layers:
        ap.error(f"{a.teacher} holds no actor.* keys: not a PPO checkpoint")
    teacher_hidden = tuple(int(sd[f"{net}.{i}.weight"].shape[0]) for i in layers[:-1])
    rkw = {}
    if a.recurrent:
        has_memory = any(k.startswith(("memory_a.", "memory_t.")) for k in sd)
        if has_memory == a.mlp_teacher:
            ap.error(f"{a.teacher} holds " + ("a recurrent teacher: drop --mlp-teacher" if has_memory else "no memory_a.* keys: a feed-forward teacher goes with --mlp-teacher"))
        H = int(sd["memory_a.rnn.weight_hh_l0" if "memory_a.rnn.weight_hh_l0" in sd else "memory_t.rnn.weight_hh_l0"].shape[1]) if has_memory else 256
        rkw = dict(rnn_type="lstm", rnn_hidden_dim=H, teacher_recurrent=has_memory)
    elif any(k.startswith("memory_a.") for k in sd):
        ap.error(f"{a.teacher} is a recurrent PPO checkpoint: pass --recurrent")
    env = ManagerBasedRLEnv(a.task, num_envs=a.num_envs, seed=a.seed, device="cuda:0")
    print(env, flush=True)
    tr = DistillTrainer(env, num_steps_per_env=120, student_hidden=(128, 128, 128), teacher_hidden=teacher_hidden, init_noise_std=0.1, learner=a.learner,
                        teacher_obs_normalization=any(k.startswith("actor_obs_normalizer.") for k in sd), seed=a.seed,
                        num_learning_epochs=2, gradient_length=15, learning_rate=1e-3, **rkw)
    resumed = tr.load_state_dict(sd)
    print(tr, f"teacher {teacher_hidden} from {a.teacher}" + (" (a distillation checkpoint: resumed)" if resumed else ""), flush=True)
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (a.num_envs,), generator=torch.Generator().manual_seed(a.seed))
    log = []
    t0 = time.perf_counter()
    for it in range(a.iterations):
        row = tr.iterate()
        log.append(row)
        print(f"it {it:4d}  behavior loss {row['behavior']:.6f}  reward/step {row['mean_reward']:+.4f}  done/step {row['done_rate']:.4f}  "
              f"grad norm {row['grad_norm']:.3e}  lr {row['learning_rate']:.1e}", flush=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    steps = a.iterations * 120 * a.num_envs
    print(json.dumps(dict(task=a.task, learner=a.learner, recurrent=a.recurrent, teacher_recurrent=bool(rkw.get("teacher_recurrent")), num_envs=a.num_envs, iterations=a.iterations, wall_s=wall, env_steps_per_s=steps / wall,
                          behavior_first=log[0]["behavior"], behavior_last=log[-1]["behavior"], falling=log[-1]["behavior"] < log[0]["behavior"])))
    if a.save:
        opt = tr.alg.optimizer_state_dict() if a.learner == "hip" else tr.alg.optimizer.state_dict()
        torch.save({"model_state_dict": tr.state_dict(), "optimizer_state_dict": opt, "iter": a.iterations, "infos": None}, a.save)
    env.close()


if __name__ == "__main__":
    main()
