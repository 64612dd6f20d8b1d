#!/usr/bin/env python
"""Time of one PPO update (5 epochs x 4 mini-batches) on ONE collected batch, both learners from the same process on the same box:

    torch: robot_lab_amd/ppo.py `PPO.update` (autograd, the update rule's definition)
    hip:   robot_lab_amd/ppo_hip.py `HipPPO.update` (csrc/rl_ppo.hip)

The batch is collected once by the HIP collector with a freshly initialised policy; then the two learners are timed ALTERNATELY
(torch, hip, torch, hip, ...) with device events around each `update()` - which ends in the learner's own read-back of the statistics, so
the host-side cost of each learner is inside its window - after `--warmup` untimed updates of each.  Reported per learner: median,
min, max over `--repeat` updates, in ms; and the algorithmic FLOPs of an update (forward + dX + dW of both networks, computed from
the shapes) over the median.  One JSON line per task and symmetry setting.

`--symmetry off lr lr,fb`: the same measurement with symmetry data augmentation inside the update (`PPO(symmetry=...)`, `HipPPO(symmetry=...)`),
both learners with the SAME tables, every setting on the same collected batch in the same process.  The tables are those of
`symmetry.tables_for_env`; for a robot it has none for (the humanoids) the timing uses random signed permutations with as many copies
("tables": "random" in the output) - the cost of the gather does not depend on which permutation it is.  Reported beside the times: the HIP
time over n_sym x the HIP time of the "off" setting of the same run, when "off" is among the settings.

`--mirror-loss C`: every `--symmetry` entry other than "off" is timed three times - the augmentation alone, the augmentation + the mirror
loss with coefficient C, the mirror loss alone (`data_augmentation=False`: only the actor sees the copies) - and each line carries
`hip_over_off`, the HIP time as a multiple of the "off" setting's.
`--split`: a third learner in the same alternation, "hip_split": `HipPPO(group=...)` with a world of ONE whose all-reduce does nothing - the
host-driven rl_ppo_update_begin / rl_ppo_minibatch_local / rl_ppo_minibatch_apply sequence of a multi-GPU run without the collective, beside the
fused `rl_ppo_update` ("hip").  `split_over_fused` is what the split itself costs: one more small launch per mini-batch and a host that
issues every mini-batch through Python instead of running ahead inside one library call.
`--obs-normalization scratch|learner`: both observation groups normalised (`Trainer(actor_obs_normalization=True, critic_obs_normalization=True)`).
"scratch": every timed update starts with the normalisation pass over the stored rows (`NormalizedBatch.normalize`, inside the window) and the
learners read its matrices; "learner" (`normalize_in_learner=True`): the learners read the raw storage - torch through the modules' forward, HIP
in its first layer's operand fetch (`HipPPO(obs_normalizers=...)`).  "scratch" is timed with symmetry "off" only: mirroring rows that were
normalised before is not the rule, and the Trainer refuses it.
`--recurrent [--rnn-hidden-dim H]`: the recurrent update (LSTM of H = 256 in front of 128-128-128 heads, 5 epochs x 4 blocks of whole trajectories) on one
batch collected by the recurrent collector: `recurrent.RecurrentPPO.update` (torch autograd through time) against `recurrent_hip.HipRecurrentPPO.update`
(csrc/learner/rl_bptt.inl), the same alternation; the FLOPs are those of the recurrence, its backward and the heads.  The other switches do not apply.
    python tools/bench_update.py [--task ID ...] [--num-envs N ...] [--repeat R] [--warmup W] [--symmetry off|lr|fb|lr,fb ...] [--mirror-loss C] [--split]
                                 [--obs-normalization scratch|learner] [--recurrent [--rnn-hidden-dim H]]"""
import argparse
import copy
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robot_lab_amd.env import ManagerBasedRLEnv  # noqa: E402
from robot_lab_amd.ppo import PPO, Trainer  # noqa: E402
from robot_lab_amd.ppo_hip import HipPPO  # noqa: E402
from robot_lab_amd.symmetry import SymmetryTables, parse_mirrors, tables_for_env  # noqa: E402


def update_flops(alg: HipPPO, rows: int, n_sym: int = 1) -> float:
    """2 flops per multiply-add x (forward + dW for every layer, dX for every layer but the first) x rows x epochs; the actor's rows are the
    n_sym copies, the critic's too unless the learner runs the mirror loss without the augmentation"""
    flops = 0.0
    for dims, copies in ((alg.actor_dims, n_sym), (alg.critic_dims, n_sym if alg.data_augmentation else 1)):
        macs = sum(dims[l] * dims[l + 1] * (3 if l > 0 else 2) for l in range(len(dims) - 1))
        flops += 2.0 * macs * rows * copies * alg.num_learning_epochs
    return flops


def tables(env, spec, dims):
    """(SymmetryTables | None, "off" | "derived" | "random")"""
    if spec == "off":
        return None, "off"
    try:
        return tables_for_env(env, spec), "derived"
    except ValueError as e:
        if "parse neither" not in str(e):  # only the documented case - a robot whose joint names give no mirror tables - falls back
            raise
        print(f"# {spec}: no derived tables for this robot ({str(e)[:60]}...): timing RANDOM signed permutations instead", file=sys.stderr, flush=True)
        n_sym, rng = 2 ** len(parse_mirrors(spec)), np.random.default_rng(0)

        def rnd(dim):
            perm = np.stack([np.arange(dim)] + [rng.permutation(dim) for _ in range(n_sym - 1)]).astype(np.int32)
            return perm, np.concatenate([np.ones((1, dim)), rng.choice([-1.0, 1.0], size=(n_sym - 1, dim))]).astype(np.float32)

        return SymmetryTables(obs=rnd(dims[0]), critic=rnd(dims[1]), act=rnd(dims[2])), "random"


class WorldOfOne:
    """the group of `--split`: enabled, so that HipPPO takes the split sequence; one rank, so that there is nothing to reduce"""

    world_size, enabled = 1, True

    def all_reduce_sum(self, tensor):
        return tensor


def bench(task, num_envs, repeat, warmup, symmetry=("off",), seed=42, mirror_loss=None, split=False, obs_normalization=None):
    env = ManagerBasedRLEnv(task, num_envs=num_envs, seed=seed, device="cuda:0")
    norm = dict(actor_obs_normalization=True, critic_obs_normalization=True, normalize_in_learner=obs_normalization == "learner") if obs_normalization else {}
    tr = Trainer(env, seed=seed, **norm)
    tr.collector.collect()
    torch.cuda.synchronize()
    out, hip_off = [], None
    for spec in symmetry:
        if obs_normalization == "scratch" and spec != "off":
            print(f"# --obs-normalization scratch with symmetry {spec}: not timed (the mirror of a normalised row is not the rule; use learner)", file=sys.stderr, flush=True)
            continue
        tab, kind = tables(env, spec, (tr.storage.observations.shape[-1], tr.storage.privileged_observations.shape[-1], env.num_actions))
        settings = [{}]  # keywords of both learners beside symmetry=
        if tab is not None and mirror_loss is not None:
            settings += [dict(mirror_loss=mirror_loss), dict(mirror_loss=mirror_loss, data_augmentation=False)]
        for kw in settings:
            res = bench_one(tr, tab, repeat, warmup, seed, split=split, **kw)
            res = dict(task=task, num_envs=num_envs, symmetry=spec, tables=kind, n_sym=tab.n_sym if tab else 1, **res)
            if obs_normalization:
                res["obs_normalization"] = obs_normalization
            if mirror_loss is not None:
                res.update(mirror_loss=kw.get("mirror_loss"), data_augmentation=kw.get("data_augmentation", True))
            if spec == "off":
                hip_off = res["hip"]["median_ms"]
            elif hip_off:
                res["hip_over_n_sym_x_off"] = res["hip"]["median_ms"] / (res["n_sym"] * hip_off)
                if mirror_loss is not None:
                    res["hip_over_off"] = res["hip"]["median_ms"] / hip_off
            out.append(res)
    env.close()
    return out


def bench_one(tr, tab, repeat, warmup, seed, split=False, **kw):
    st = tr.storage
    tr.sync_normalizers()  # (the modules the copied policies carry hold the collection's statistics)
    hip_kw = dict(kw, obs_normalizers=tr.normalizers) if tr.normalize_in_learner else kw
    learners = {"torch": PPO(copy.deepcopy(tr.policy), symmetry=tab, **kw), "hip": HipPPO(copy.deepcopy(tr.policy), symmetry=tab, **hip_kw)}
    if split:
        learners["hip_split"] = HipPPO(copy.deepcopy(tr.policy), symmetry=tab, group=WorldOfOne(), **hip_kw)
    gens = {k: torch.Generator(device="cuda:0").manual_seed(seed) for k in learners}
    times = {k: [] for k in learners}
    for it in range(warmup + repeat):
        for k, alg in learners.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            out = alg.update(tr.update_batch(), gens[k])  # (with scratch normalisation: the pass over the stored rows is part of every update)
            t1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append(t0.elapsed_time(t1))
            assert all(v == v for v in out.values()), (k, out)  # no NaN
    rows = st.num_transitions_per_env * st.num_envs
    flops = update_flops(learners["hip"], rows, tab.n_sym if tab else 1)
    res = dict(rows=rows, repeat=repeat, warmup=warmup, update_gflop=flops / 1e9)
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = dict(median_ms=med, min_ms=min(t), max_ms=max(t), tflops_at_median=flops / med / 1e9)
    res["speedup_median"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    if split:
        res["split_over_fused"] = res["hip_split"]["median_ms"] / res["hip"]["median_ms"]
        learners["hip_split"].close()
    learners["hip"].close()
    return res


def bench_rnd(task, num_envs, repeat, warmup, seed=42):
    """One update with and without random network distillation (predictor / target 256-256 -> 1 on the policy group, state normalisation on) on either
    learner, the four learners alternating on ONE collected batch: median ms per update and what RND adds."""
    from robot_lab_amd.rnd_hip import HipRND

    env = ManagerBasedRLEnv(task, num_envs=num_envs, seed=seed, device="cuda:0")
    tr = Trainer(env, seed=seed, rnd=dict(weight=0.1, state_normalization=True, reward_normalization=True, predictor_hidden_dims=[256, 256], target_hidden_dims=[256, 256]))
    tr.collector.collect()
    batch = tr.update_batch()
    torch.cuda.synchronize()
    st = tr.storage
    rows = st.num_transitions_per_env * st.num_envs
    hip_rnd = HipRND(copy.deepcopy(tr.rnd), 5, 4, rows // 4, state_normalizer=tr.rnd_device.state_norm)
    learners = {"torch": PPO(copy.deepcopy(tr.policy)), "torch_rnd": PPO(copy.deepcopy(tr.policy), rnd=copy.deepcopy(tr.rnd)),
                "hip": HipPPO(copy.deepcopy(tr.policy)), "hip_rnd": HipPPO(copy.deepcopy(tr.policy), rnd=hip_rnd)}
    gens = {k: torch.Generator(device="cuda:0").manual_seed(seed) for k in learners}
    times = {k: [] for k in learners}
    for it in range(warmup + repeat):
        for k, alg in learners.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            out = alg.update(batch, gens[k])
            t1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append(t0.elapsed_time(t1))
            assert all(v == v for v in out.values()), (k, out)  # no NaN
    res = dict(task=task, num_envs=num_envs, rows=rows, repeat=repeat, warmup=warmup, rnd="256-256 -> 1, state normalisation")
    for k, t in times.items():
        res[k] = dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
    res["torch_rnd_adds_ms"] = res["torch_rnd"]["median_ms"] - res["torch"]["median_ms"]
    res["hip_rnd_adds_ms"] = res["hip_rnd"]["median_ms"] - res["hip"]["median_ms"]
    learners["hip"].close(); learners["hip_rnd"].close(); hip_rnd.close(); env.close()
    return res


def recurrent_flops(alg, rows: int) -> float:
    """2 flops per multiply-add x rows x epochs x (the memories: W_ih forward + dW, W_hh forward + dX + dW; the heads: forward + dX + dW per layer - the
    first layer's dX is dL/dh)"""
    H4 = 4 * alg.hidden
    macs = sum(H4 * D * 2 + H4 * alg.hidden * 3 for D in (alg.obs_dim, alg.critic_obs_dim))
    macs += sum(dims[l] * dims[l + 1] * 3 for dims in (alg.actor_dims, alg.critic_dims) for l in range(len(dims) - 1))
    return 2.0 * macs * rows * alg.num_learning_epochs


def bench_recurrent(task, num_envs, repeat, warmup, hidden=256, seed=42):
    from robot_lab_amd.recurrent import RecurrentPPO
    from robot_lab_amd.recurrent_hip import HipRecurrentPPO

    env = ManagerBasedRLEnv(task, num_envs=num_envs, seed=seed, device="cuda:0")
    tr = Trainer(env, seed=seed, rnn_type="lstm", rnn_hidden_dim=hidden, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128))
    env.episode_length_buf = torch.randint(0, int(env.max_episode_length), (num_envs,), generator=torch.Generator().manual_seed(seed))  # dones inside the window
    tr.collector.collect()
    torch.cuda.synchronize()
    batch, st = tr.update_batch(), tr.storage
    learners = {"torch": RecurrentPPO(copy.deepcopy(tr.policy)), "hip": HipRecurrentPPO(copy.deepcopy(tr.policy))}
    times = {k: [] for k in learners}
    for it in range(warmup + repeat):
        for k, alg in learners.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            out = alg.update(batch)
            t1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[k].append(t0.elapsed_time(t1))
            assert all(v == v for v in out.values()), (k, out)  # no NaN
    rows = st.num_transitions_per_env * (num_envs // learners["hip"].num_mini_batches) * learners["hip"].num_mini_batches
    flops = recurrent_flops(learners["hip"], rows)
    res = dict(task=task, num_envs=num_envs, recurrent=f"lstm({hidden})", rows=rows, done_rate=float(st.dones.float().mean()), repeat=repeat, warmup=warmup,
               update_gflop=flops / 1e9)
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = dict(median_ms=med, min_ms=min(t), max_ms=max(t), tflops_at_median=flops / med / 1e9)
    res["speedup_median"] = res["torch"]["median_ms"] / res["hip"]["median_ms"]
    learners["hip"].close()
    tr.recurrent.close(); env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", nargs="+", default=["RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0", "RobotLab-Isaac-Velocity-Rough-Unitree-G1-v0"])
    ap.add_argument("--num-envs", nargs="+", type=int, default=[4096, 2048])
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--symmetry", nargs="+", default=["off"], help="settings to time, each \"off\" or mirrors (lr | fb | lr,fb)")
    ap.add_argument("--mirror-loss", type=float, default=None, metavar="C", help="also time every symmetry setting with the mirror loss, with and without the augmentation")
    ap.add_argument("--split", action="store_true", help="also time the begin / local / apply sequence of a multi-GPU run at a world of one")
    ap.add_argument("--obs-normalization", choices=("scratch", "learner"), default=None,
                    help="normalise both observation groups: in a pass before every update (scratch) or inside the learners (learner)")
    ap.add_argument("--recurrent", action="store_true", help="time the recurrent update: the torch rule against the HIP learner's back-propagation through time")
    ap.add_argument("--rnn-hidden-dim", type=int, default=256)
    ap.add_argument("--rnd", action="store_true", help="time one update with and without random network distillation on either learner")
    a = ap.parse_args()
    if a.rnd:
        if a.symmetry != ["off"] or a.mirror_loss is not None or a.split or a.obs_normalization or a.recurrent:
            ap.error("--rnd does not combine with --symmetry, --mirror-loss, --split, --obs-normalization or --recurrent (Trainer(rnd=...) refuses them)")
        if len(a.num_envs) != len(a.task):
            ap.error("one --num-envs per --task")
        for task, n in zip(a.task, a.num_envs):
            print(json.dumps(bench_rnd(task, n, a.repeat, a.warmup)), flush=True)
        return
    if a.recurrent:
        if a.symmetry != ["off"] or a.mirror_loss is not None or a.split or a.obs_normalization:
            ap.error("--recurrent does not combine with --symmetry, --mirror-loss, --split or --obs-normalization (the recurrent learners refuse them)")
        if len(a.num_envs) != len(a.task):
            ap.error("one --num-envs per --task")
        for task, n in zip(a.task, a.num_envs):
            print(json.dumps(bench_recurrent(task, n, a.repeat, a.warmup, a.rnn_hidden_dim)), flush=True)
        return
    for spec in a.symmetry:
        if spec != "off":
            parse_mirrors(spec)
    if len(a.num_envs) != len(a.task):
        ap.error("one --num-envs per --task")
    for task, n in zip(a.task, a.num_envs):
        for res in bench(task, n, a.repeat, a.warmup, a.symmetry, mirror_loss=a.mirror_loss, split=a.split, obs_normalization=a.obs_normalization):
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
