#!/usr/bin/env python
"""The data-collection half of one PPO iteration as the reference runs it through `runner.learn(...)`
(scripts/reinforcement_learning/rsl_rl/train.py:224; rsl_rl OnPolicyRunner.learn): for each of `num_steps_per_env`
(= 24) steps  actions = alg.act(obs); obs, rewards, dones, extras = env.step(actions); alg.process_env_step(...),
then alg.compute_returns(obs) - every piece on the HIP kernels of this repo (actor + critic: rl_policy.hip, noise /
log-prob / storage / GAE: rl_rollout.hip, env: rl_env.hip).  Random network weights: the arithmetic does not
depend on them.
    python tools/bench_collect.py [task] [num_envs] [iterations] [--obs-history N] [--obs-normalization] [--recurrent]
--obs-history N: policy-group observation history of N frames, measured against history off in alternating windows of this process.
--obs-normalization: empirical normalisation of both groups (csrc/rl_obsnorm.hip) against the fused-act loop and against the unfused loop
(actor + critic, then the act kernel) it is built on, alternating windows of this process.
--recurrent: the recurrent loop (two LSTM cells of H = 256 in one launch, csrc/rl_lstm.hip, in front of 128-128-128 heads, unfused act) against the
feed-forward fused-act loop (512-256-128 networks) and the feed-forward unfused loop, alternating windows of this process.
--rnd: random network distillation behind every env.step (csrc/rl_rnd.hip; predictor and target 256-256 -> 1 on the policy group) without and with
both of its normalisers, against the fused-act loop it is built on, alternating windows of this process."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from robot_lab_amd.env import ManagerBasedRLEnv  # noqa: E402
from robot_lab_amd.policy import MlpPolicy  # noqa: E402
from robot_lab_amd.rollout import RolloutStorage  # noqa: E402

ap_hist = 0
if "--obs-history" in sys.argv:  # --obs-history N: policy-group observation history (rl_env_set_obs_history); runs history off / on alternating in this process
    i = sys.argv.index("--obs-history")
    ap_hist = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
ap_norm = "--obs-normalization" in sys.argv
if ap_norm:
    sys.argv.remove("--obs-normalization")
ap_rec = "--recurrent" in sys.argv
if ap_rec:
    sys.argv.remove("--recurrent")
ap_rnd = "--rnd" in sys.argv
if ap_rnd:
    sys.argv.remove("--rnd")
task = sys.argv[1] if len(sys.argv) > 1 else "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 40
T, GAMMA, LAM = 24, 0.99, 0.95  # rsl_rl_ppo_cfg.py:11,33-34
FUSED = os.environ.get("RL_FUSED_RECORD", "1") == "1"
PAIR = os.environ.get("RL_PAIR", "1") == "1"  # actor + critic in one launch (rl_mlp_forward_pair)
GRAPH = os.environ.get("RL_GRAPH", "1") == "1"  # the whole iteration as one hipGraph launch (robot_lab_amd/collect.py)
SMALL = os.environ.get("RL_CRITIC_SMALL", "1") == "1"  # (overlap) the critic through rl_mlp_forward_small
FUSED_ACT = os.environ.get("RL_FUSED_ACT", "1") == "1"  # sampling / log-prob / the slot's first half in the actor + critic launch's epilogue (0: the act kernel)
OVERLAP = os.environ.get("RL_OVERLAP", "0") == "1"  # the critic of step t on a second stream under env step t (0: actor + critic as one launch in front of act)


def setup(hist, norm=False, fused_act=FUSED_ACT, recurrent=False, rnd=None):
    """-> (env, storage, iteration(obs) -> obs) of one collection loop; `hist`: policy-group history length (0: none); `norm`: both groups normalised;
    `recurrent`: LSTM cells of H = 256 in front of 128-128-128 heads (the reference's recurrent agent cfgs)"""
    env = ManagerBasedRLEnv(task, num_envs=N, seed=42, device="cuda:0", obs_history={"policy": hist} if hist else None)
    obs, _ = env.reset()
    od, cd, A = obs["policy"].shape[1], obs["critic"].shape[1], env.num_actions
    rng = np.random.default_rng(0)

    def net(dims):
        ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
        return MlpPolicy(ws, [np.zeros(d, dtype=np.float32) for d in dims[1:]], "elu", device="cuda:0")

    actor, critic = (net([256, 128, 128, 128, A]), net([256, 128, 128, 128, 1])) if recurrent else (net([od, 512, 256, 128, A]), net([cd, 512, 256, 128, 1]))
    std = torch.ones(A, device="cuda:0")  # init_noise_std = 1.0 (rsl_rl_ppo_cfg.py:16)
    storage = RolloutStorage(N, T, od, cd, A, seed=1, device="cuda:0")
    if recurrent:
        from robot_lab_amd.collect import Collector  # noqa: E402
        from robot_lab_amd.lstm import LstmCell, RecurrentState  # noqa: E402

        def cell(D, H=256):  # nn.LSTM's default initialisation
            u = lambda *s: rng.uniform(-1 / np.sqrt(H), 1 / np.sqrt(H), s).astype(np.float32)  # noqa: E731
            return LstmCell(u(4 * H, D), u(4 * H, H), u(4 * H), u(4 * H), device="cuda:0")

        rec = RecurrentState(cell(od), cell(cd), N, T)
        col = Collector(env, actor, critic, storage, std, GAMMA, LAM, use_graph=True, recurrent=rec)
        return env, storage, (lambda obs: col.collect()), (actor, critic, col, rec)
    if rnd is not None:  # `rnd`: normalisers on / off; rsl_rl's defaults otherwise (one output), 256-256 networks on the policy group
        from robot_lab_amd.collect import Collector  # noqa: E402
        from robot_lab_amd.rnd import RandomNetworkDistillation  # noqa: E402
        from robot_lab_amd.rnd_hip import RndDevice  # noqa: E402

        torch.manual_seed(0)
        module = RandomNetworkDistillation(od, num_outputs=1, predictor_hidden_dims=(256, 256), target_hidden_dims=(256, 256), weight=0.1, state_normalization=rnd,
                                           reward_normalization=rnd).to("cuda:0")
        dev = RndDevice(module, N, T, device="cuda:0")
        col = Collector(env, actor, critic, storage, std, GAMMA, LAM, use_graph=True, rnd=dev)
        return env, storage, (lambda obs: col.collect()), (actor, critic, col, dev)
    if GRAPH and FUSED and PAIR:
        from robot_lab_amd.collect import Collector  # noqa: E402

        normalizers = None
        if norm:
            from robot_lab_amd.obsnorm import ObsNormalizer  # noqa: E402

            normalizers = (ObsNormalizer(od, max_rows=N, device="cuda:0"), ObsNormalizer(cd, max_rows=N, device="cuda:0"))
        col = Collector(env, actor, critic, storage, std, GAMMA, LAM, use_graph=True, overlap=OVERLAP, critic_small=SMALL, fused_act=fused_act, normalizers=normalizers)
        return env, storage, (lambda obs: col.collect()), (actor, critic, col, normalizers)
    if norm:
        raise SystemExit("--obs-normalization measures the captured loop: leave RL_GRAPH, RL_FUSED_RECORD and RL_PAIR at 1")

    def iteration(obs):
        storage.clear()
        for _ in range(T):
            mean, values = actor.forward_pair(obs["policy"], critic, obs["critic"]) if PAIR else (actor(obs["policy"]), critic(obs["critic"]))
            actions = storage.act(obs["policy"], obs["critic"], mean, std, values)
            if FUSED:  # the env kernel writes the transition's rewards / dones into the storage slot (rl_env_step_record)
                obs, rew, term, tout, extras = env.step(actions, rollout=storage, gamma=GAMMA)
            else:
                obs, rew, term, tout, extras = env.step(actions)
                storage.process_env_step(rew, term, tout, GAMMA)
        storage.compute_returns(critic(obs["critic"]), GAMMA, LAM)
        return obs

    return env, storage, iteration, (actor, critic)


def window(iteration, obs, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        obs = iteration(obs)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, obs


if ap_hist > 0:
    # history off and on, alternating steady-state windows in ONE process: us per step of the collection loop and of a bare env.step()
    # loop (zero actions), every window listed with the spread of each side
    ROUNDS, STEPS = 6, 4000  # a window of either loop is 0.2 - 0.6 s of device time
    sides = {}
    with torch.inference_mode():
        for h in (0, ap_hist):
            env, storage, iteration, keep = setup(h)
            obs = env.get_observations()
            for _ in range(3):
                obs = iteration(obs)
            zero = torch.zeros(N, env.num_actions, device="cuda:0")
            sides[h] = dict(env=env, storage=storage, iteration=iteration, keep=keep, obs=obs, zero=zero, collect=[], step=[])
        for r in range(ROUNDS):
            for h in ((0, ap_hist) if r % 2 == 0 else (ap_hist, 0)):
                sd = sides[h]
                dt, sd["obs"] = window(sd["iteration"], sd["obs"], ITERS)
                sd["collect"].append(1e6 * dt / ITERS / T)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    sd["env"].step(sd["zero"])
                torch.cuda.synchronize()
                sd["step"].append(1e6 * (time.perf_counter() - t0) / STEPS)
    for h, sd in sides.items():
        for what in ("collect", "step"):
            v = np.array(sd[what])
            print(f"{task} N={N} obs_history={h} policy_dim={sd['obs']['policy'].shape[1]} {what:7s} us/step: windows {np.round(v, 2).tolist()} "
                  f"median {np.median(v):.2f} min {v.min():.2f} max {v.max():.2f}")
    for what in ("collect", "step"):
        off, on = np.median(sides[0][what]), np.median(sides[ap_hist][what])
        print(f"{task} N={N} {what}: history {ap_hist} costs {on - off:+.2f} us/step ({100 * (on - off) / off:+.1f} %) over history off (medians of {ROUNDS} alternating windows)")
    ok = all(bool(torch.isfinite(sd["storage"].advantages).all()) for sd in sides.values())
    print(f"finite: {ok}")
    sys.exit(0 if ok else 1)

if ap_norm:
    # fused-act loop (the default), the unfused loop (actor + critic, act kernel) and the normalised loop (apply_pair, actor + critic, act kernel,
    # env step, update_pair), alternating steady-state windows in ONE process: us per step of the collection loop, every window listed
    ROUNDS = 6
    kinds = {"fused_act": dict(norm=False, fused_act=True), "unfused_act": dict(norm=False, fused_act=False), "normalized": dict(norm=True)}
    sides = {}
    with torch.inference_mode():
        for name, kw in kinds.items():
            env, storage, iteration, keep = setup(0, **kw)
            obs = env.get_observations()
            for _ in range(3):
                obs = iteration(obs)
            sides[name] = dict(env=env, storage=storage, iteration=iteration, keep=keep, obs=obs, collect=[])
        order = list(kinds)
        for r in range(ROUNDS):
            for name in (order if r % 2 == 0 else order[::-1]):
                sd = sides[name]
                dt, sd["obs"] = window(sd["iteration"], sd["obs"], ITERS)
                sd["collect"].append(1e6 * dt / ITERS / T)
    for name, sd in sides.items():
        v = np.array(sd["collect"])
        print(f"{task} N={N} {name:12s} collect us/step: windows {np.round(v, 2).tolist()} median {np.median(v):.2f} min {v.min():.2f} max {v.max():.2f}")
    med = {name: float(np.median(sd["collect"])) for name, sd in sides.items()}
    print(f"{task} N={N}: normalisation costs {med['normalized'] - med['fused_act']:+.2f} us/step ({100 * (med['normalized'] - med['fused_act']) / med['fused_act']:+.1f} %) over the "
          f"fused-act loop: {med['unfused_act'] - med['fused_act']:+.2f} for the act kernel as a launch of its own, {med['normalized'] - med['unfused_act']:+.2f} for apply_pair + update_pair "
          f"(medians of {ROUNDS} alternating windows)")
    count = int(sides["normalized"]["keep"][3][0].get_state()[3])
    ok = all(bool(torch.isfinite(sd["storage"].advantages).all()) for sd in sides.values()) and count > 0
    print(f"finite: {ok}; rows seen by the policy group's statistics: {count}")
    sys.exit(0 if ok else 1)

if ap_rnd:
    # the fused-act loop (RND off), RND without normalisers (2 launches per step more: the predictor / target pair, the one reward kernel) and RND with
    # both normalisers (6 more: + state update and apply, + the dim-1 update with avg and the finish kernel), alternating steady-state windows in ONE process
    ROUNDS = 6
    kinds = {"rnd_off": dict(), "rnd": dict(rnd=False), "rnd_normalized": dict(rnd=True)}
    sides = {}
    with torch.inference_mode():
        for name, kw in kinds.items():
            env, storage, iteration, keep = setup(0, **kw)
            obs = env.get_observations()
            for _ in range(3):
                obs = iteration(obs)
            sides[name] = dict(env=env, storage=storage, iteration=iteration, keep=keep, obs=obs, collect=[])
        order = list(kinds)
        for r in range(ROUNDS):
            for name in (order if r % 2 == 0 else order[::-1]):
                sd = sides[name]
                dt, sd["obs"] = window(sd["iteration"], sd["obs"], ITERS)
                sd["collect"].append(1e6 * dt / ITERS / T)
    for name, sd in sides.items():
        v = np.array(sd["collect"])
        print(f"{task} N={N} {name:15s} collect us/step: windows {np.round(v, 2).tolist()} median {np.median(v):.2f} min {v.min():.2f} max {v.max():.2f}")
    med = {name: float(np.median(sd["collect"])) for name, sd in sides.items()}
    print(f"{task} N={N}: RND costs {med['rnd'] - med['rnd_off']:+.2f} us/step ({100 * (med['rnd'] - med['rnd_off']) / med['rnd_off']:+.1f} %) over the fused-act loop "
          f"(the pair launch + the reward kernel), {med['rnd_normalized'] - med['rnd_off']:+.2f} ({100 * (med['rnd_normalized'] - med['rnd_off']) / med['rnd_off']:+.1f} %) with both "
          f"normalisers (+ update, apply, update of the reward statistics, finish) (medians of {ROUNDS} alternating windows)")
    sums = sides["rnd_normalized"]["keep"][3].reward.sums()
    ok = all(bool(torch.isfinite(sd["storage"].advantages).all()) for sd in sides.values()) and sums[0] > 0
    print(f"finite: {ok}; mean intrinsic reward of the last iteration {sums[0] / (T * N):.4f}")
    sys.exit(0 if ok else 1)

if ap_rec:
    # feed-forward fused-act loop (the default), feed-forward unfused loop and the recurrent loop, alternating steady-state windows in ONE process
    ROUNDS = 6
    kinds = {"fused_act": dict(fused_act=True), "unfused_act": dict(fused_act=False), "recurrent": dict(recurrent=True)}
    sides = {}
    with torch.inference_mode():
        for name, kw in kinds.items():
            env, storage, iteration, keep = setup(0, **kw)
            obs = env.get_observations()
            for _ in range(3):
                obs = iteration(obs)
            sides[name] = dict(env=env, storage=storage, iteration=iteration, keep=keep, obs=obs, collect=[])
        order = list(kinds)
        for r in range(ROUNDS):
            for name in (order if r % 2 == 0 else order[::-1]):
                sd = sides[name]
                dt, sd["obs"] = window(sd["iteration"], sd["obs"], ITERS)
                sd["collect"].append(1e6 * dt / ITERS / T)
    for name, sd in sides.items():
        v = np.array(sd["collect"])
        print(f"{task} N={N} {name:12s} collect us/step: windows {np.round(v, 2).tolist()} median {np.median(v):.2f} min {v.min():.2f} max {v.max():.2f}")
    med = {name: float(np.median(sd["collect"])) for name, sd in sides.items()}
    print(f"{task} N={N}: the recurrent loop costs {med['recurrent'] - med['fused_act']:+.2f} us/step ({100 * (med['recurrent'] - med['fused_act']) / med['fused_act']:+.1f} %) over the "
          f"feed-forward fused-act loop, {med['recurrent'] - med['unfused_act']:+.2f} over the feed-forward unfused loop (medians of {ROUNDS} alternating windows)")
    rec = sides["recurrent"]["keep"][3]
    ok = all(bool(torch.isfinite(sd["storage"].advantages).all()) for sd in sides.values()) and bool((rec.h_a != 0).any()) and bool(torch.isfinite(rec.h_c).all())
    print(f"finite: {ok}")
    sys.exit(0 if ok else 1)

env, storage, iteration, _keep = setup(0)
obs = env.get_observations()
with torch.inference_mode():
    for _ in range(3):
        obs = iteration(obs)
    dt, obs = window(iteration, obs, ITERS)
ok = bool(torch.isfinite(storage.advantages).all() and torch.isfinite(storage.returns).all())
print(f"{task} N={N} graph={int(GRAPH and FUSED and PAIR)} overlap={int(OVERLAP and GRAPH and FUSED and PAIR)} critic_small={int(SMALL)}: collection of {T} steps + GAE {1e3 * dt / ITERS:.3f} ms / iteration = {N * T * ITERS / dt / 1e6:.1f} M env-steps/s "
      f"({1e6 * dt / ITERS / T:.1f} us / step; finite: {ok}; adv mean {float(storage.advantages.mean()):+.2e} std {float(storage.advantages.std()):.4f})")
