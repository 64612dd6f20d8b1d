"""`OnPolicyRunner` as the reference's scripts use it (train.py:205-224, play.py:190-246):

    runner = OnPolicyRunner(env, agent_cfg.to_dict(), log_dir=log_dir, device=agent_cfg.device)
    runner.add_git_repo_to_log(__file__); runner.load(path); runner.learn(num_learning_iterations=..., init_at_random_ep_len=True)
    policy = runner.get_inference_policy(device=...); runner.alg.policy  (exporters, `.reset(dones)`)

`env` is the `RslRlVecEnvWrapper` of the shims around `robot_lab_amd.env.ManagerBasedRLEnv`.  Collection runs on the HIP kernels as
one hipGraph launch per iteration (robot_lab_amd/collect.py), the update is robot_lab_amd/ppo.py - or, with `RL_LEARNER=hip` in the
environment, the HIP learner of robot_lab_amd/ppo_hip.py, on one GPU or under `--distributed` -, checkpoints use rsl_rl's layout
(`model_<it>.pt`: model_state_dict / optimizer_state_dict / iter / infos) with either learner, and one learner's checkpoint resumes the other.
`policy.actor_obs_normalization` / `policy.critic_obs_normalization` reach the `Trainer` (csrc/rl_obsnorm.hip); the checkpoint then carries
rsl_rl's `actor_obs_normalizer.*` / `critic_obs_normalizer.*` buffers.
A recurrent cfg - `policy.class_name="ActorCriticRecurrent"`, or the reference's `actor=` / `critic=` RNNModel cfgs (robot_lab_amd.recurrent.read_recurrent_cfg) -
builds `Trainer(rnn_type="lstm", ...)`: the LSTM cells run in the captured collection (csrc/rl_lstm.hip), the update is the torch learner's or - with
`RL_RECURRENT_LEARNER=hip` in the environment - back-propagation through time on the HIP learner of robot_lab_amd/recurrent_hip.py; checkpoints carry
rsl_rl's `memory_a.rnn.*` / `memory_c.rnn.*` keys, `get_inference_policy()` is stateful with `reset(dones)`.
`algorithm.rnd_cfg` (IsaacLab's `RslRlRndCfg` fields) with `obs_groups["rnd_state"]` builds `Trainer(rnd=...)`: random network distillation with either learner;
checkpoints then carry rsl_rl's `rnd_state_dict` / `rnd_optimizer_state_dict`."""
from __future__ import annotations

import os
import time

import torch


def learner_from_env(environ=None) -> str:
    """`RL_LEARNER=torch | hip` (default torch: robot_lab_amd.ppo.PPO); anything else is refused, never read as the default"""
    value = (os.environ if environ is None else environ).get("RL_LEARNER", "torch")
    if value not in ("torch", "hip"):
        raise ValueError(f"RL_LEARNER={value!r}: the learner is \"torch\" (robot_lab_amd.ppo.PPO, the default) or \"hip\" (robot_lab_amd.ppo_hip.HipPPO)")
    return value


def recurrent_learner_from_env(environ=None) -> str:
    """`RL_RECURRENT_LEARNER=torch | hip` (default torch: robot_lab_amd.recurrent.RecurrentPPO), read with a recurrent cfg; anything else is refused"""
    value = (os.environ if environ is None else environ).get("RL_RECURRENT_LEARNER", "torch")
    if value not in ("torch", "hip"):
        raise ValueError(f"RL_RECURRENT_LEARNER={value!r}: the recurrent learner is \"torch\" (robot_lab_amd.recurrent.RecurrentPPO, the default) or \"hip\" "
                         "(robot_lab_amd.recurrent_hip.HipRecurrentPPO)")
    return value


class OnPolicyRunner:
    def __init__(self, env, train_cfg: dict, log_dir: str | None = None, device: str = "cpu"):
        from robot_lab_amd.ppo import Trainer

        self.env, self.cfg, self.log_dir, self.device = env, train_cfg, log_dir, device
        self.learner = learner_from_env()
        from robot_lab_amd.recurrent import RecurrentInferencePolicy, read_recurrent_cfg

        pol, alg = dict(train_cfg.get("policy") or {}), dict(train_cfg.get("algorithm", {}))
        # a recurrent cfg (policy.class_name="ActorCriticRecurrent", or the reference's actor= / critic= RNNModel cfgs): the Trainer keywords, else None
        recurrent = read_recurrent_cfg(train_cfg)
        if recurrent is not None:
            if self.learner == "hip":
                raise NotImplementedError("stand-in runner: RL_LEARNER=hip with a recurrent cfg is not implemented: RL_LEARNER names the feed-forward learners, "
                                          "and back-propagation through time in the HIP learner has a switch of its own - unset RL_LEARNER and set "
                                          "RL_RECURRENT_LEARNER=hip (robot_lab_amd/recurrent_hip.py)")
            recurrent["recurrent_learner"] = recurrent_learner_from_env()
            pol = dict(class_name="ActorCritic", actor_hidden_dims=recurrent.pop("actor_hidden"), critic_hidden_dims=recurrent.pop("critic_hidden"),
                       init_noise_std=recurrent.pop("init_noise_std"), noise_std_type=pol.get("noise_std_type", "scalar"))
        if pol.get("class_name", "ActorCritic") != "ActorCritic" or alg.get("class_name", "PPO") != "PPO":
            raise NotImplementedError(f"stand-in runner: ActorCritic + PPO only, got {pol.get('class_name')} / {alg.get('class_name')}")
        if pol.get("activation", "elu") != "elu":
            raise NotImplementedError("stand-in runner: ELU networks only (what every robot_lab agent cfg uses)")
        # rsl_rl's empirical observation normalisation per group: robot_lab_amd.ppo.EmpiricalNormalization on csrc/rl_obsnorm.hip
        norm = dict(actor_obs_normalization=bool(pol.get("actor_obs_normalization")), critic_obs_normalization=bool(pol.get("critic_obs_normalization")))
        sym = alg.get("symmetry_cfg")
        if sym:
            get = sym.get if isinstance(sym, dict) else lambda k, d=None: getattr(sym, k, d)  # noqa: E731
            mirror = ", mirror_loss=<mirror_loss_coeff>, data_augmentation=<use_data_augmentation>" if get("use_mirror_loss") else ""
            raise NotImplementedError("stand-in runner: a symmetry_cfg carries an arbitrary Python data_augmentation_func, which cannot be turned into the "
                                      "learners' tables; symmetry data augmentation and the mirror loss inside the update are "
                                      f"robot_lab_amd.ppo.Trainer(env, symmetry=\"lr\" | \"lr,fb\" | SymmetryTables{mirror}) (INTEGRATION.md section 7)")
        # random network distillation: `algorithm.rnd_cfg` (IsaacLab's RslRlRndCfg fields) + `obs_groups["rnd_state"]` -> Trainer(rnd=...); what it does
        # not combine with is refused by the reader / the Trainer with a reason (robot_lab_amd/rnd.py)
        from robot_lab_amd.rnd import read_rnd_cfg

        rnd = read_rnd_cfg(train_cfg)
        # options this stand-in does not implement are refused, never ignored (a silently different learner is worse than none)
        groups = dict(train_cfg.get("obs_groups") or {})
        actor_set = groups.get("policy", groups.get("actor", ["policy"]))
        if recurrent is None and (list(actor_set) != ["policy"] or list(groups.get("critic", ["critic"])) != ["critic"]):
            raise NotImplementedError(f"stand-in runner: obs_groups {groups} - only policy <- ['policy'], critic <- ['critic'] (what every "
                                      f"robot_lab velocity cfg but ANYmal-D's uses) is wired to the fused inference kernels")
        if pol.get("noise_std_type", "scalar") != "scalar":
            raise NotImplementedError(f"stand-in runner: noise_std_type={pol.get('noise_std_type')!r}; the sampling kernel reads a scalar-type std vector")
        if train_cfg.get("empirical_normalization"):
            raise NotImplementedError("stand-in runner: the runner-level empirical_normalization is rsl_rl's deprecated spelling and is not read here: set "
                                      "policy.actor_obs_normalization=True and policy.critic_obs_normalization=True, which mean the same")
        if alg.get("normalize_advantage_per_mini_batch"):
            raise NotImplementedError("stand-in runner: normalize_advantage_per_mini_batch is not implemented")
        # one process per GPU (README.md:323-337, train.py:143-150): rsl_rl's multi-GPU contract lives in robot_lab_amd/dist.py.  A world of
        # N ranks whose learners were not tied together would be N unrelated trainings writing over each other's logs - never run that.
        from robot_lab_amd.dist import LearnerGroup

        self.group = LearnerGroup(device)
        keys = ("value_loss_coef", "use_clipped_value_loss", "clip_param", "entropy_coef", "num_learning_epochs", "num_mini_batches",
                "learning_rate", "schedule", "desired_kl", "max_grad_norm")
        self.trainer = Trainer(env.unwrapped, num_steps_per_env=int(train_cfg.get("num_steps_per_env", 24)), gamma=float(alg.get("gamma", 0.99)),
                               lam=float(alg.get("lam", 0.95)), seed=int(train_cfg.get("seed", 42)), actor_hidden=pol.get("actor_hidden_dims", (512, 256, 128)),
                               critic_hidden=pol.get("critic_hidden_dims", (512, 256, 128)), init_noise_std=float(pol.get("init_noise_std", 1.0)),
                               clip_actions=getattr(env, "clip_actions", None), group=self.group if self.group.enabled else None, learner=self.learner,
                               **{k: v for k, v in norm.items() if v}, **(recurrent or {}), **({"rnd": rnd} if rnd is not None else {}),
                               **{k: alg[k] for k in keys if k in alg})
        self.alg = self.trainer.alg
        # the learner keeps master parameters and Adam's state on the device (HipPPO, or - RL_RECURRENT_LEARNER=hip - HipRecurrentPPO: the same methods)
        self._device_learner = self.learner == "hip" or (recurrent is not None and recurrent.get("recurrent_learner") == "hip")
        self._inference = None
        if recurrent is not None:  # one stateful callable: `runner.alg.policy.reset(dones)` and the inference policy's `reset` are the same state
            self._inference = RecurrentInferencePolicy(self.trainer.recurrent.cell_a, self.trainer.actor)
            self.alg.policy.reset = self._inference.reset
        else:
            self.alg.policy.reset = lambda dones=None: None  # feed-forward policy: nothing to reset (play.py:246)
        self.save_interval = int(train_cfg.get("save_interval", 50))
        self.current_learning_iteration = 0
        self.git_status_repos = []
        self.last_episode_log = None  # rank 0: extras["log"] with the means over every rank's envs (robot_lab_amd/dist.py reduce_episode_log)

    def add_git_repo_to_log(self, path):
        self.git_status_repos.append(path)

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False):
        env = self.env.unwrapped
        if init_at_random_ep_len:
            env.episode_length_buf = torch.randint(0, int(env.max_episode_length), (env.num_envs,))
        main = self.group.is_main  # rank 0 logs and writes checkpoints, the other ranks train silently (rsl_rl `disable_logs`)
        if self.log_dir and main:
            os.makedirs(self.log_dir, exist_ok=True)
        start = self.current_learning_iteration
        t0 = time.time()
        for it in range(start, start + num_learning_iterations):
            out = self.trainer.iterate()
            self.current_learning_iteration = it + 1
            steps = self.trainer.storage.num_transitions_per_env * env.num_envs * self.group.world_size
            # the episode log of the JOB, not of rank 0's envs: the packed episode-metric vector SUM all-reduced over the ranks on a side
            # stream (every rank takes part in the collective, rank 0 alone reads the result)
            # Only at the log interval (`self.log_interval`, default every iteration as rsl_rl prints every iteration), and every rank
            # keeps its handle until the next collective and resolves it then (`vector()`: work.wait() + stream order) - a rank must not
            # drop an async Work handle while its tensor is in flight.
            from robot_lab_amd.dist import reduce_episode_log

            if getattr(self, "_log_in_flight", None) is not None:
                self._log_in_flight.vector()
                self._log_in_flight = None
            if (it + 1 - start) % max(1, int(getattr(self, "log_interval", 1))) != 0 and it + 1 != start + num_learning_iterations:
                continue
            episode_log = reduce_episode_log(env)
            if not main:
                self._log_in_flight = episode_log
                continue
            self.last_episode_log = ep = episode_log.result()
            print(f"[rsl_rl stand-in] iteration {it + 1}/{start + num_learning_iterations}  mean reward/step {out['mean_reward']:+.4f}  value loss {out['value_loss']:.4f}  "
                  f"surrogate {out['surrogate_loss']:+.4f}  std {out['action_std']:.3f}  lr {out['learning_rate']:.1e}  "
                  + (f"rnd loss {out['rnd_loss']:.3e}  intrinsic {out['mean_intrinsic_reward']:+.4f}  extrinsic {out['mean_extrinsic_reward']:+.4f}  "
                     f"rnd weight {out['rnd_weight']:.3g}  " if "rnd_loss" in out else "") +
                  f"{steps * (it + 1 - start) / max(time.time() - t0, 1e-9):.0f} steps/s  "
                  f"episode log over {int(ep['num_envs'])} envs ({int(ep['episodes'])} episodes ended)"
                  + (f"  terrain level {float(ep['Curriculum/terrain_levels']):.2f}" if "Curriculum/terrain_levels" in ep else ""), flush=True)
            if self.log_dir and (it + 1) % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it + 1}.pt"))
        if getattr(self, "_log_in_flight", None) is not None:
            self._log_in_flight.vector()
            self._log_in_flight = None
        if self.log_dir and main:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
        if self._device_learner:
            self.alg.store_into(self.alg.policy)  # `runner.alg.policy` is current after learn(), as the torch learner's is (exporters, play.py)

    def save(self, path: str, infos=None):
        if self._device_learner:  # the master parameters and Adam's state live on the device: into the module / torch.optim.Adam's layout
            self.alg.store_into(self.alg.policy)
            optimizer_state = self.alg.optimizer_state_dict()
        else:
            optimizer_state = self.alg.optimizer.state_dict()
        self.trainer.sync_normalizers()  # the running statistics live on the device: into the module's buffers (rsl_rl's keys)
        saved = {"model_state_dict": self.alg.policy.state_dict(), "optimizer_state_dict": optimizer_state,
                 "iter": self.current_learning_iteration, "infos": infos}
        if self.trainer.rnd is not None:  # rsl_rl's keys; the optimiser's in torch.optim.Adam's layout with either learner
            saved["rnd_state_dict"] = self.trainer.rnd_state_dict()
            saved["rnd_optimizer_state_dict"] = self.trainer.rnd_optimizer_state_dict()
        torch.save(saved, path)

    def load(self, path: str, load_optimizer: bool = True, map_location=None):
        d = torch.load(path, map_location=map_location or self.trainer.device, weights_only=False)
        self.alg.policy.load_state_dict(d["model_state_dict"])  # strict: normaliser keys the flags do not ask for - or miss - raise here
        if self.trainer.rnd is not None:
            if "rnd_state_dict" not in d:
                raise KeyError(f"{path} has no rnd_state_dict: it was written by a run without rnd_cfg")
            self.trainer.load_rnd_state(d["rnd_state_dict"], d.get("rnd_optimizer_state_dict") if load_optimizer else None)
        if self._device_learner:
            self.alg.load_from(self.alg.policy)
            if load_optimizer and d.get("optimizer_state_dict"):
                self.alg.load_optimizer_state_dict(d["optimizer_state_dict"])
        elif load_optimizer and d.get("optimizer_state_dict"):
            self.alg.optimizer.load_state_dict(d["optimizer_state_dict"])
            if self._inference is not None:  # recurrent: the adaptive schedule continues from the checkpoint's rate, so a resumed run repeats the original's steps
                self.alg.learning_rate = float(self.alg.optimizer.param_groups[0]["lr"])
        self.current_learning_iteration = int(d.get("iter", 0))
        self.trainer.push_parameters()  # (the normalisers' buffers go to their handles with it)
        return d.get("infos")

    def get_inference_policy(self, device=None):
        if self._inference is not None:  # recurrent: the actor's cell (csrc/rl_lstm.hip) and MLP head, stateful, with `reset(dones)`
            return self._inference
        actor = self.trainer.actor  # the fused HIP inference kernel (csrc/rl_policy.hip), fed by push_parameters()
        norm = (self.trainer.normalizers or (None, None))[0]  # the actor group's statistics are applied, never updated (rsl_rl `act_inference`)

        def policy(obs):
            obs = obs if torch.is_tensor(obs) else obs["policy"]
            if norm is not None:
                obs = norm.apply(obs.to(device=norm.device, dtype=torch.float32).contiguous())
            return actor(obs)

        return policy


def _given(d, key, default=None):
    """d[key], with a cfg field that was never filled in (`dataclasses.MISSING`, None) read as `default`"""
    from dataclasses import MISSING

    v = d.get(key, default)
    return default if v is None or v is MISSING else v


def read_distillation_cfg(train_cfg: dict, env_groups=("policy", "critic")) -> dict:
    """The keywords of `robot_lab_amd.distill.DistillTrainer` from a `RslRlDistillationRunnerCfg.to_dict()` in the reference file's spelling
    (`.../anymal_d/agents/rsl_rl_distillation_cfg.py`).  What this stand-in does not implement is refused with a reason, never ignored."""
    if "policy" in train_cfg and _given(train_cfg, "policy") is not None:
        raise NotImplementedError("stand-in DistillationRunner: `policy=dict(class_name=\"StudentTeacher\", ...)` is rsl_rl 3.0.1's spelling and is not read "
                                  "here: give the two networks as `student` / `teacher` model cfgs (RslRlMLPModelCfg), as the reference's "
                                  "rsl_rl_distillation_cfg.py does")
    models = {}
    for role in ("student", "teacher"):
        m = _given(train_cfg, role)
        if not isinstance(m, dict):
            raise ValueError(f"stand-in DistillationRunner: the cfg has no `{role}` model cfg (RslRlMLPModelCfg: hidden_dims, activation, obs_normalization, distribution_cfg)")
        if _given(m, "rnn_type") is not None or m.get("class_name") == "RNNModel":
            raise NotImplementedError(f"stand-in DistillationRunner: the {role} is a recurrent model (rnn_type={m.get('rnn_type')!r}); recurrent students and "
                                      "teachers are not implemented - use the feed-forward RslRlMLPModelCfg")
        if _given(m, "activation", "elu") != "elu":
            raise NotImplementedError(f"stand-in DistillationRunner: {role} activation={m.get('activation')!r}; ELU networks only (the fused inference kernels "
                                      "and the HIP learner implement ELU)")
        if _given(m, "hidden_dims") is None:
            raise ValueError(f"stand-in DistillationRunner: the {role} model cfg has no hidden_dims")
        models[role] = m
    if _given(models["student"], "obs_normalization", False):
        raise NotImplementedError("stand-in DistillationRunner: student obs_normalization=True is not implemented (the student's statistics would have to be "
                                  "updated inside the captured collection loop and applied in the learner); set it to False")
    alg = _given(train_cfg, "algorithm", {})
    if alg.get("class_name", "Distillation") != "Distillation":
        raise NotImplementedError(f"stand-in DistillationRunner: algorithm.class_name={alg.get('class_name')!r}, only \"Distillation\"")
    if _given(alg, "optimizer", "adam") != "adam":
        raise NotImplementedError(f"stand-in DistillationRunner: optimizer={alg.get('optimizer')!r}; only \"adam\" (torch.optim.Adam's defaults, which the HIP "
                                  "learner's step kernel implements)")
    groups = dict(_given(train_cfg, "obs_groups", {}) or {})
    chosen = {}
    for role in ("student", "teacher"):
        sets = list(groups.get(role, ["policy"]))
        if len(sets) != 1:
            raise NotImplementedError(f"stand-in DistillationRunner: obs_groups[{role!r}] = {sets}: exactly one observation group per network is wired to the "
                                      "fused inference kernels (no concatenation of groups)")
        if sets[0] not in env_groups:
            raise ValueError(f"stand-in DistillationRunner: obs_groups[{role!r}] = {sets}: the env has no observation group {sets[0]!r} (it has {sorted(env_groups)})")
        chosen[role] = sets[0]
    dist = _given(models["student"], "distribution_cfg", {}) or {}
    kw = dict(num_steps_per_env=int(_given(train_cfg, "num_steps_per_env", 24)), student_hidden=tuple(models["student"]["hidden_dims"]),
              teacher_hidden=tuple(models["teacher"]["hidden_dims"]), init_noise_std=float(_given(dist, "init_std", 0.1)),
              student_group=chosen["student"], teacher_group=chosen["teacher"],
              teacher_obs_normalization=bool(_given(models["teacher"], "obs_normalization", False)), seed=int(_given(train_cfg, "seed", 42)),
              num_learning_epochs=int(_given(alg, "num_learning_epochs", 1)), gradient_length=int(_given(alg, "gradient_length", 15)),
              learning_rate=float(_given(alg, "learning_rate", 1e-3)), max_grad_norm=_given(alg, "max_grad_norm"), loss_type=_given(alg, "loss_type", "mse"))
    return kw


def _is_rnn_model(m) -> bool:
    return isinstance(m, dict) and (_given(m, "rnn_type") is not None or m.get("class_name") == "RNNModel")


def is_recurrent_distillation_cfg(train_cfg: dict) -> bool:
    """whether a distillation runner cfg asks for a recurrent student or teacher (`RslRlRNNModelCfg`).  Pure."""
    return any(_is_rnn_model(_given(train_cfg, role)) for role in ("student", "teacher"))


def read_recurrent_distillation_cfg(train_cfg: dict, env_groups=("policy", "critic")) -> dict:
    """The keywords of `robot_lab_amd.distill.DistillTrainer` from the reference's recurrent distillation cfg
    (`AnymalDFlatDistillationRunnerRecurrentCfg.to_dict()`): the student an RNNModel, the teacher an RNNModel with equal rnn settings or an MLPModel.
    Every other refusal is `read_distillation_cfg`'s, which reads the cfg with the rnn fields taken out.  Pure (no device, no env)."""
    from robot_lab_amd.recurrent import check_rnn_cfg

    models = {role: _given(train_cfg, role) for role in ("student", "teacher")}
    for role, m in models.items():
        if not isinstance(m, dict):
            raise ValueError(f"stand-in DistillationRunner: the cfg has no `{role}` model cfg (RslRlRNNModelCfg / RslRlMLPModelCfg)")
    if not _is_rnn_model(models["student"]):
        raise NotImplementedError("stand-in DistillationRunner: the teacher is a recurrent model and the student is not: a feed-forward student with a recurrent "
                                  "teacher is not implemented (out of scope) - make the student an RslRlRNNModelCfg too, or distil a feed-forward teacher")
    rnn = {}
    for role, m in models.items():
        if not _is_rnn_model(m):
            continue
        if m.get("class_name", "RNNModel") != "RNNModel" or _given(m, "rnn_type") is None:
            raise NotImplementedError(f"stand-in DistillationRunner: the {role} is {m.get('class_name')!r} with rnn_type={m.get('rnn_type')!r}: a recurrent model is "
                                      "class_name=\"RNNModel\" with an rnn_type")
        rnn[role] = (_given(m, "rnn_type"), int(_given(m, "rnn_hidden_dim", 256)), int(_given(m, "rnn_num_layers", 1)))
        check_rnn_cfg(f"stand-in DistillationRunner ({role})", *rnn[role])
    if "teacher" in rnn and rnn["teacher"] != rnn["student"]:
        raise NotImplementedError(f"stand-in DistillationRunner: student and teacher rnn settings differ ({rnn['student']} / {rnn['teacher']}): "
                                  "StudentTeacherRecurrent has one rnn_type / rnn_hidden_dim / rnn_num_layers for both memories")
    plain = dict(train_cfg)
    for role, m in models.items():  # the feed-forward reader sees MLP models: its refusals (activation, normalisation, algorithm, optimiser, groups) apply unchanged
        plain[role] = {k: v for k, v in m.items() if k not in ("rnn_type", "rnn_hidden_dim", "rnn_num_layers")}
        if plain[role].get("class_name") == "RNNModel":
            plain[role]["class_name"] = "MLPModel"
    kw = read_distillation_cfg(plain, env_groups)
    kw.update(rnn_type=rnn["student"][0], rnn_hidden_dim=rnn["student"][1], rnn_num_layers=rnn["student"][2], teacher_recurrent="teacher" in rnn)
    return kw


class DistillationRunner:
    """rsl_rl's `DistillationRunner` as the reference's scripts use it (train.py:205-217): the same calls as `OnPolicyRunner`.  Collection is
    robot_lab_amd/distill_collect.py (student and teacher in one launch, one hipGraph launch per iteration), the update robot_lab_amd/distill.py
    or - `RL_LEARNER=hip` - robot_lab_amd/distill_hip.py.  `load(path)` goes through `StudentTeacher.load_state_dict`: a PPO checkpoint becomes the
    teacher (iteration 0, fresh optimiser), a distillation checkpoint resumes iteration and optimiser.  Checkpoints are `model_<it>.pt` in rsl_rl's layout.
    A cfg with RNNModel networks (`is_recurrent_distillation_cfg`) gives the recurrent student of robot_lab_amd/distill_recurrent.py: the same calls,
    `load()` of a recurrent PPO checkpoint gives the teacher, `get_inference_policy()` the stateful callable with `reset(dones)`."""

    def __init__(self, env, train_cfg: dict, log_dir: str | None = None, device: str = "cpu"):
        from robot_lab_amd.dist import LearnerGroup, rank_info
        from robot_lab_amd.distill import DistillTrainer

        world = rank_info()[2]
        if world > 1:  # before a process group is formed: the other ranks would wait for a collective that never comes
            raise NotImplementedError(f"stand-in DistillationRunner: a LearnerGroup of {world} ranks is not implemented (the distillation "
                                      "learners do not exchange gradients): run one rank")
        self.env, self.cfg, self.log_dir, self.device = env, train_cfg, log_dir, device
        self.learner = learner_from_env()
        inner = env.unwrapped
        self.recurrent = is_recurrent_distillation_cfg(train_cfg)
        kw = (read_recurrent_distillation_cfg if self.recurrent else read_distillation_cfg)(train_cfg, tuple(inner.get_observations().keys()))
        self.group = LearnerGroup(device)  # (a world of one: disabled, no process group)
        self.trainer = DistillTrainer(inner, learner=self.learner, clip_actions=_given(train_cfg, "clip_actions", getattr(env, "clip_actions", None)), **kw)
        self.alg = self.trainer.alg
        self.save_interval = int(_given(train_cfg, "save_interval", 50))
        self.current_learning_iteration = 0
        self.git_status_repos = []
        self.history = []  # the statistics of every iteration of learn()

    def add_git_repo_to_log(self, path):
        self.git_status_repos.append(path)

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False):
        if not self.alg.policy.loaded_teacher:
            raise ValueError("DistillationRunner.learn: no teacher is loaded - call load(<PPO checkpoint of the teacher>) first (train.py does, for "
                             "every Distillation cfg)")
        env = self.env.unwrapped
        if init_at_random_ep_len:
            env.episode_length_buf = torch.randint(0, int(env.max_episode_length), (env.num_envs,))
        if self.log_dir:
            os.makedirs(self.log_dir, exist_ok=True)
        start = self.current_learning_iteration
        t0 = time.time()
        for it in range(start, start + num_learning_iterations):
            out = self.trainer.iterate()
            self.history.append(out)
            self.current_learning_iteration = it + 1
            steps = self.trainer.storage.num_transitions_per_env * env.num_envs
            print(f"[rsl_rl stand-in] distillation {it + 1}/{start + num_learning_iterations}  behavior loss {out['behavior']:.6f}  mean reward/step "
                  f"{out['mean_reward']:+.4f}  grad norm {out['grad_norm']:.3e}  lr {out['learning_rate']:.1e}  "
                  f"{steps * (it + 1 - start) / max(time.time() - t0, 1e-9):.0f} steps/s", flush=True)
            if self.log_dir and (it + 1) % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it + 1}.pt"))
        if self.log_dir:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))
        if self.learner == "hip":
            self.alg.store_into(self.alg.policy)  # `runner.alg.policy` is current after learn() (exporters, play.py)

    def save(self, path: str, infos=None):
        if self.learner == "hip":
            self.alg.store_into(self.alg.policy)
            optimizer_state = self.alg.optimizer_state_dict()
        else:
            optimizer_state = self.alg.optimizer.state_dict()
        torch.save({"model_state_dict": self.alg.policy.state_dict(), "optimizer_state_dict": optimizer_state,
                    "iter": self.current_learning_iteration, "infos": infos}, path)

    def load(self, path: str, load_optimizer: bool = True, map_location=None):
        d = torch.load(path, map_location=map_location or self.trainer.device, weights_only=False)
        resumed = self.trainer.load_state_dict(d["model_state_dict"])
        if resumed:  # a distillation checkpoint: iteration and optimiser continue; a teacher's PPO checkpoint starts at 0 with a fresh optimiser
            if load_optimizer and d.get("optimizer_state_dict"):
                if self.learner == "hip":
                    self.alg.load_optimizer_state_dict(d["optimizer_state_dict"])
                else:
                    self.alg.optimizer.load_state_dict(d["optimizer_state_dict"])
            self.current_learning_iteration = int(d.get("iter", 0))
        return d.get("infos")

    def get_inference_policy(self, device=None):
        if self.recurrent:  # stateful: policy(obs) advances the student's memory, policy.reset(dones) zeroes rows (play.py calls it after env.step)
            return self.trainer.inference_policy()
        student = self.trainer.student  # the fused HIP inference kernel, fed by the push after every update

        def policy(obs):
            obs = obs if torch.is_tensor(obs) else obs[self.trainer.student_group]
            return student(obs)

        return policy
