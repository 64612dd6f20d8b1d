#!/usr/bin/env python
"""Time of one distillation update on ONE collected batch, both learners from the same process on the same box, and of the collection loop with
and without the captured graph:

    torch: robot_lab_amd/distill.py `Distillation.update` (autograd, the rule's definition)
    hip:   robot_lab_amd/distill_hip.py `HipDistillation.update` (csrc/learner/rl_distill.inl on the PPO learner's kernels)

The reference cfg's size (rsl_rl_distillation_cfg.py) on A1 Rough: 4096 envs x 120 steps, gradient length 15, two epochs, student 128-128-128;
the teacher is a randomly initialised 512-256-128 actor.  The batch is collected once; the two learners are then timed ALTERNATELY (torch, hip,
torch, hip, ...) with device events around each `update()` - which ends in the learner's own read-back of the statistics - after `--warmup`
untimed updates of each.  The collection is timed the same way: `--repeat` iterations of the eager loop and of the captured replay, alternating.
Medians, minima and maxima in ms; one JSON line, and a text report to `--out`.
`--recurrent`: the reference's recurrent cfg instead - an LSTM of 256 in front of student and teacher (128-128-128 each; `--mlp-teacher`: a
feed-forward 512-256-128 teacher), `RecurrentDistillation` against `HipRecurrentDistillation` (csrc/learner/rl_distill_bptt.inl), the collection
with the two memories.
    python tools/bench_distill.py [--recurrent [--mlp-teacher]] [--task ID] [--num-envs N] [--steps T] [--repeat R] [--warmup W] [--out FILE]"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robot_lab_amd.distill import Distillation, DistillTrainer  # noqa: E402
from robot_lab_amd.distill_hip import HipDistillation  # noqa: E402
from robot_lab_amd.env import ManagerBasedRLEnv  # noqa: E402
from robot_lab_amd.ppo import ActorCritic  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), n=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recurrent", action="store_true", help="an LSTM student (and teacher): robot_lab_amd/distill_recurrent.py")
    ap.add_argument("--mlp-teacher", action="store_true", help="with --recurrent: a feed-forward teacher")
    a = ap.parse_args()
    if a.mlp_teacher and not a.recurrent:
        ap.error("--mlp-teacher goes with --recurrent")
    kw = dict(num_learning_epochs=2, gradient_length=15, learning_rate=1e-3)
    rnn_teacher = a.recurrent and not a.mlp_teacher
    teacher_hidden = (128, 128, 128) if rnn_teacher else (512, 256, 128)
    rkw = dict(rnn_type="lstm", rnn_hidden_dim=256, teacher_recurrent=rnn_teacher) if a.recurrent else {}
    trainers = {}
    for graph in (False, True):  # two envs with the same seed: the eager loop and the captured one
        env = ManagerBasedRLEnv(a.task, num_envs=a.num_envs, seed=1, device="cuda:0")
        tr = DistillTrainer(env, num_steps_per_env=a.steps, student_hidden=(128, 128, 128), teacher_hidden=teacher_hidden, init_noise_std=0.1, learner="torch",
                            use_graph=graph, seed=1, **rkw, **kw)
        torch.manual_seed(2)
        od = env.get_observations()["policy"].shape[1]
        if rnn_teacher:
            from robot_lab_amd.recurrent import ActorCriticRecurrent

            tr.load_state_dict(ActorCriticRecurrent(od, od, env.num_actions).state_dict())
        else:
            tr.load_state_dict(ActorCritic(od, od, env.num_actions, actor_hidden=teacher_hidden).state_dict())
        trainers[graph] = tr
    for _ in range(max(a.warmup, 2)):  # (the captured side: eager warm-up, then capture + replay)
        for tr in trainers.values():
            tr.collector.collect()
    torch.cuda.synchronize()
    collect = {False: [], True: []}
    for _ in range(a.repeat):
        for graph, tr in trainers.items():
            collect[graph].append(timed(tr.collector.collect))
    tr = trainers[True]
    batch = tr.batch
    if a.recurrent:
        from robot_lab_amd.distill_recurrent import RecurrentDistillation
        from robot_lab_amd.distill_recurrent_hip import HipRecurrentDistillation

        learners = dict(torch=RecurrentDistillation(copy.deepcopy(tr.policy), **kw), hip=HipRecurrentDistillation(copy.deepcopy(tr.policy), num_envs=a.num_envs, **kw))
    else:
        learners = dict(torch=Distillation(copy.deepcopy(tr.policy), **kw), hip=HipDistillation(copy.deepcopy(tr.policy), num_envs=a.num_envs, **kw))
    for _ in range(a.warmup):
        for alg in learners.values():
            alg.update(batch)
    times = {k: [] for k in learners}
    for _ in range(a.repeat):
        for k, alg in learners.items():
            times[k].append(timed(lambda: alg.update(batch)))  # noqa: B023
    out = dict(task=a.task, num_envs=a.num_envs, steps=a.steps, student=[128, 128, 128], recurrent=a.recurrent, teacher_recurrent=rnn_teacher,
               **{k: v for k, v in kw.items()},
               optimiser_steps_per_update=learners["hip"].num_updates, update={k: spread(v) for k, v in times.items()},
               hip_over_torch=statistics.median(times["hip"]) / statistics.median(times["torch"]),
               collect=dict(eager=spread(collect[False]), graph=spread(collect[True])),
               collect_us_per_step=dict(eager=1e3 * statistics.median(collect[False]) / a.steps, graph=1e3 * statistics.median(collect[True]) / a.steps))
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"tools/bench_distill.py{' --recurrent' if a.recurrent else ''}{' --mlp-teacher' if a.mlp_teacher else ''}: {a.task}, {a.num_envs} envs x "
                    f"{a.steps} steps, student {'LSTM 256 + ' if a.recurrent else ''}128-128-128, gradient length 15, 2 epochs "
                    f"({out['optimiser_steps_per_update']} optimiser steps per update); {a.repeat} alternating windows after {a.warmup} warm-up updates\n")
            for k, v in out["update"].items():
                f.write(f"update   {k:<6} median {v['median_ms']:9.3f} ms   min {v['min_ms']:9.3f}   max {v['max_ms']:9.3f}\n")
            f.write(f"update   hip / torch (medians) {out['hip_over_torch']:.3f}\n")
            for k, v in out["collect"].items():
                f.write(f"collect  {k:<6} median {v['median_ms']:9.3f} ms   min {v['min_ms']:9.3f}   max {v['max_ms']:9.3f}   {out['collect_us_per_step'][k]:8.2f} us / step\n")
            f.write(json.dumps(out) + "\n")
    for t in trainers.values():
        t.env.close()


if __name__ == "__main__":
    main()
