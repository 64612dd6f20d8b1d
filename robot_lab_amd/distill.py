"""Teacher-student distillation, the second half of rsl_rl's "train a teacher with PPO, then distil it" recipe, without the (absent) rsl-rl-lib:

    collect (HIP: student + teacher in ONE launch, sampling head, storage, env - robot_lab_amd/distill_collect.py, one hipGraph launch)
    -> update (this file: torch autograd; or robot_lab_amd/distill_hip.py: the same rule as HIP kernels) -> push the student into the
    inference kernel in place -> collect ...

What the reference gets from `train.py --agent=rsl_rl_distillation_cfg_entry_point --load_run <teacher>` (scripts/reinforcement_learning/
rsl_rl/train.py:205-217 -> rsl_rl `DistillationRunner.learn` -> `Distillation.update`) with `.../anymal_d/agents/rsl_rl_distillation_cfg.py`.
This module restates rsl_rl's `StudentTeacher` and `Distillation` for feed-forward networks and is THE DEFINITION of the rule here, as
`ppo.py` is for PPO; `tests/test_distill.py` checks it against its definition on an exact integer family.

    policy = StudentTeacher(obs_dim, teacher_obs_dim, act_dim, student_hidden, teacher_hidden, init_noise_std)
    policy.load_state_dict(torch.load(teacher_checkpoint)["model_state_dict"])   # a PPO checkpoint: actor.* -> teacher.*; returns False
    alg = Distillation(policy, num_learning_epochs=2, gradient_length=15, learning_rate=1e-3)
    alg.update(batch)        # batch.observations [T, N, obs_dim], batch.teacher_actions [T, N, act_dim] -> {"behavior": mean loss}
"""
from __future__ import annotations

import types

import torch
from torch import nn

from .ppo import MAX_INPUT_WIDTH, EmpiricalNormalization, mlp

LOSS_TYPES = ("mse", "huber")


class StudentTeacher(nn.Module):
    """rsl_rl `StudentTeacher` for feed-forward ELU networks.  Submodules in rsl_rl's order - `student`, `teacher` (eval mode, never
    differentiated), `std`, optionally `teacher_obs_normalizer` (applied, never updated) -, so `state_dict()` keys are rsl_rl's:
    `student.<2l>.weight|bias`, `teacher.<2l>.weight|bias`, `std`, `teacher_obs_normalizer.*`."""

    def __init__(self, obs_dim, teacher_obs_dim, act_dim, student_hidden=(128, 128, 128), teacher_hidden=(512, 256, 128), init_noise_std=0.1,
                 teacher_obs_normalization=False):
        super().__init__()
        self.loaded_teacher = False
        self.student = mlp([obs_dim, *student_hidden, act_dim])
        self.teacher = mlp([teacher_obs_dim, *teacher_hidden, act_dim])
        self.teacher.eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)
        self.std = nn.Parameter(init_noise_std * torch.ones(act_dim))
        self.teacher_obs_normalization = bool(teacher_obs_normalization)
        if teacher_obs_normalization:
            self.teacher_obs_normalizer = EmpiricalNormalization(teacher_obs_dim)
            self.teacher_obs_normalizer.eval()  # (`update` does nothing outside training mode)
        else:
            self.teacher_obs_normalizer = nn.Identity()

    def train(self, mode=True):
        super().train(mode)
        self.teacher.eval()
        self.teacher_obs_normalizer.eval()
        return self

    def reset(self, dones=None):
        pass

    def act(self, obs):
        mean = self.student(obs)
        return mean + self.std * torch.randn_like(mean)

    def act_inference(self, obs):
        return self.student(obs)

    @torch.no_grad()
    def evaluate(self, teacher_obs):
        return self.teacher(self.teacher_obs_normalizer(teacher_obs))

    def load_state_dict(self, state_dict, strict=True):
        """Three cases.  A PPO checkpoint (any key starts with `actor.`; this project's or rsl_rl's): `actor.*` -> `teacher.*`, strict on names
        and shapes, `actor_obs_normalizer.*` -> `teacher_obs_normalizer.*` (a normaliser on one side only is an error); returns False ("not a
        resume").  A distillation checkpoint (keys start with `student.`): loaded strictly; returns True.  Anything else is an error."""
        keys = list(state_dict.keys())
        if any(k.startswith("actor.") for k in keys):
            teacher = {k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}
            norm = {k[len("actor_obs_normalizer."):]: v for k, v in state_dict.items() if k.startswith("actor_obs_normalizer.")}
            if bool(norm) != self.teacher_obs_normalization:
                raise RuntimeError("StudentTeacher.load_state_dict: the PPO checkpoint " + ("carries" if norm else "has no") + " actor_obs_normalizer.* but this "
                                   "policy was built with teacher_obs_normalization=" + str(self.teacher_obs_normalization) + ": the teacher would see rows "
                                   "it was not trained on (build the policy with teacher_obs_normalization=" + str(bool(norm)) + ")")
            self.teacher.load_state_dict(teacher, strict=True)
            if norm:
                self.teacher_obs_normalizer.load_state_dict(norm, strict=True)
            self.loaded_teacher = True
            self.teacher.eval()
            return False
        if any(k.startswith("student.") for k in keys):
            super().load_state_dict(state_dict, strict=True)
            self.loaded_teacher = True
            self.teacher.eval()
            return True
        raise ValueError("StudentTeacher.load_state_dict: the state dict has neither actor.* (a PPO checkpoint, which becomes the teacher) nor "
                         f"student.* (a distillation checkpoint) keys: {keys[:6]}")


def behavior_loss(loss_type):
    if loss_type == "mse":
        return nn.functional.mse_loss
    if loss_type == "huber":
        return nn.functional.huber_loss  # (default delta = 1)
    raise ValueError(f"Distillation: unknown loss_type {loss_type!r} (\"mse\" or \"huber\")")


def update_groups(T, gradient_length, num_learning_epochs):
    """The time steps of every optimiser step of one `Distillation.update`, and the left-over steps: cnt runs ACROSS the epochs."""
    seq = [t for _ in range(num_learning_epochs) for t in range(T)]
    full = len(seq) // gradient_length
    return [tuple(seq[i * gradient_length:(i + 1) * gradient_length]) for i in range(full)], tuple(seq[full * gradient_length:])


class Distillation:
    """rsl_rl `Distillation` on a filled batch of T steps x N envs: `batch.observations` [T, N, obs_dim] (the student's rows) and
    `batch.teacher_actions` [T, N, act_dim].  Only the student ever receives a gradient."""

    def __init__(self, policy: StudentTeacher, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse"):
        if num_learning_epochs < 1 or gradient_length < 1:
            raise ValueError("Distillation: num_learning_epochs and gradient_length must be >= 1")
        self.policy = policy
        self.num_learning_epochs, self.gradient_length, self.learning_rate, self.max_grad_norm = num_learning_epochs, gradient_length, learning_rate, max_grad_norm
        self.loss_type, self.loss_fn = loss_type, behavior_loss(loss_type)
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate)
        self.last_grad_norm = float("nan")
        self.grad_norms = []  # the pre-clip gradient norms of the last update, one per optimiser step
        self.num_updates = 0

    def update(self, batch) -> dict:
        obs, teacher_actions = batch.observations, batch.teacher_actions
        self.grad_norms = []
        student = self.policy.student
        cnt, loss, total = 0, 0, 0.0
        for _ in range(self.num_learning_epochs):
            for t in range(obs.shape[0]):  # time order, whole steps
                l_t = self.loss_fn(student(obs[t]), teacher_actions[t])  # the mean over the N * act_dim entries
                loss = loss + l_t
                total += float(l_t.detach())
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    norm = nn.utils.clip_grad_norm_(student.parameters(), self.max_grad_norm if self.max_grad_norm else float("inf"))
                    self.last_grad_norm = float(norm)
                    self.grad_norms.append(self.last_grad_norm)
                    self.optimizer.step()
                    self.num_updates += 1
                    loss = 0
        return {"behavior": total / cnt}


def student_shapes(dims):
    """shapes of `student.parameters()` (= the flat layout of include/rl_distill.h): W, b per layer"""
    return [s for l in range(len(dims) - 1) for s in ((dims[l + 1], dims[l]), (dims[l + 1],))]


class DistillTrainer:
    """collect (HIP, one graph launch) -> update -> push the student, repeated: `DistillationRunner.learn` in miniature.
    `learner="torch"`: `Distillation` above; `learner="hip"`: `distill_hip.HipDistillation`, the same rule as HIP kernels.
    `student_group` / `teacher_group`: which of the env's observation groups ("policy" | "critic") each network reads.
    `teacher_obs_normalization`: the teacher was trained behind an `actor_obs_normalizer`; its statistics come with the teacher's
    checkpoint, are applied in front of the teacher and never updated.  The teacher arrives through `load_state_dict` / `load_teacher`.
    `rnn_type="lstm"` (with `rnn_hidden_dim`, `rnn_num_layers=1`): a recurrent student, robot_lab_amd/distill_recurrent.py - `StudentTeacherRecurrent`,
    `RecurrentDistillation` or `distill_recurrent_hip.HipRecurrentDistillation`, `RecurrentDistillCollector`.  `teacher_recurrent` (None: as the
    student): the teacher has a memory of its own (a recurrent PPO checkpoint) or is feed-forward.  `carry_learner_state`: after an update the
    collection's student state becomes the learner's `final_state`; False: the collection continues from its own cells."""

    def __init__(self, env, num_steps_per_env=120, student_hidden=(128, 128, 128), teacher_hidden=(512, 256, 128), init_noise_std=0.1, learner="torch",
                 student_group="policy", teacher_group="policy", teacher_obs_normalization=False, clip_actions=None, seed=1, use_graph=True,
                 rnn_type=None, rnn_hidden_dim=256, rnn_num_layers=1, teacher_recurrent=None, carry_learner_state=True, **distillation_kw):
        from .distill_collect import DistillCollector
        from .policy import MlpPolicy
        from .rollout import RolloutStorage

        if learner not in ("torch", "hip"):
            raise ValueError(f"learner must be \"torch\" or \"hip\", not {learner!r}")
        self.recurrent = rnn_type is not None
        if self.recurrent:  # (refused before the env is touched)
            from .recurrent import check_rnn_cfg

            check_rnn_cfg("DistillTrainer", rnn_type, rnn_hidden_dim, rnn_num_layers)
            teacher_recurrent = True if teacher_recurrent is None else bool(teacher_recurrent)
        elif teacher_recurrent:
            raise NotImplementedError("DistillTrainer: teacher_recurrent=True without rnn_type= means a feed-forward student with a recurrent teacher, which is "
                                      "not implemented (out of scope: the collection runs the teacher's memory next to the student's); pass rnn_type=\"lstm\" "
                                      "for a recurrent student, or teacher_recurrent=False with a feed-forward PPO checkpoint")
        self.teacher_recurrent, self.carry_learner_state = bool(teacher_recurrent), bool(carry_learner_state)
        obs, _ = env.reset()
        for role, g in (("student", student_group), ("teacher", teacher_group)):
            if g not in obs:
                raise ValueError(f"DistillTrainer: the {role}'s observation group {g!r} is not one of the env's ({sorted(obs.keys())})")
            if obs[g].shape[1] > MAX_INPUT_WIDTH:
                raise ValueError(f"DistillTrainer: the {g} observation row is {obs[g].shape[1]} columns wide, the fused inference kernels and the HIP "
                                 f"learner take at most {MAX_INPUT_WIDTH} input columns")
        sd, td, A = obs[student_group].shape[1], obs[teacher_group].shape[1], env.num_actions
        torch.manual_seed(seed)
        self.env, self.device, self.learner = env, obs[student_group].device, learner
        self.student_group, self.teacher_group = student_group, teacher_group
        if self.recurrent:
            self._init_recurrent(env, sd, td, A, num_steps_per_env, tuple(student_hidden), tuple(teacher_hidden), init_noise_std, teacher_obs_normalization,
                                 clip_actions, seed, use_graph, int(rnn_hidden_dim), distillation_kw)
            return
        self.policy = StudentTeacher(sd, td, A, tuple(student_hidden), tuple(teacher_hidden), init_noise_std, teacher_obs_normalization).to(self.device)
        if learner == "hip":
            from .distill_hip import HipDistillation

            self.alg = HipDistillation(self.policy, num_envs=env.num_envs, **distillation_kw)
        else:
            self.alg = Distillation(self.policy, **distillation_kw)
        lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        self.student = MlpPolicy([host(x.weight) for x in lin(self.policy.student)], [host(x.bias) for x in lin(self.policy.student)], "elu", device=str(self.device))
        self.teacher = MlpPolicy([host(x.weight) for x in lin(self.policy.teacher)], [host(x.bias) for x in lin(self.policy.teacher)], "elu", device=str(self.device))
        self.normalizer = None
        if teacher_obs_normalization:
            from .obsnorm import ObsNormalizer

            m = self.policy.teacher_obs_normalizer
            self.normalizer = ObsNormalizer(m._mean.shape[1], m.eps, max_rows=env.num_envs, device=str(self.device))
        self.storage = RolloutStorage(env.num_envs, num_steps_per_env, sd, td, A, seed=seed, device=str(self.device))
        self.std = self.policy.std.detach().clone()  # the tensor the sampling kernel reads (std is not trained: it keeps its value)
        self.collector = DistillCollector(env, self.student, self.teacher, self.storage, self.std, student_group=student_group, teacher_group=teacher_group,
                                          normalizer=self.normalizer, use_graph=use_graph, clip_actions=clip_actions)
        self.batch = types.SimpleNamespace(observations=self.storage.observations, teacher_actions=self.collector.teacher_actions)
        self.iteration = 0

    def _init_recurrent(self, env, sd, td, A, num_steps_per_env, student_hidden, teacher_hidden, init_noise_std, teacher_obs_normalization, clip_actions, seed,
                        use_graph, H, distillation_kw):
        """the recurrent student's half of the constructor: memories in front of both MLPs (the teacher's only with `teacher_recurrent`)"""
        from .distill_collect import RecurrentDistillCollector
        from .distill_recurrent import RecurrentDistillation, StudentTeacherRecurrent
        from .lstm import LstmCell
        from .policy import MlpPolicy
        from .rollout import RolloutStorage

        dev = str(self.device)
        self.policy = StudentTeacherRecurrent(sd, td, A, student_hidden, teacher_hidden, init_noise_std, rnn_hidden_dim=H, teacher_recurrent=self.teacher_recurrent,
                                              teacher_obs_normalization=teacher_obs_normalization).to(self.device)
        if self.learner == "hip":
            from .distill_recurrent_hip import HipRecurrentDistillation

            self.alg = HipRecurrentDistillation(self.policy, num_envs=env.num_envs, **distillation_kw)
        else:
            self.alg = RecurrentDistillation(self.policy, **distillation_kw)
        lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        self.student = MlpPolicy([host(x.weight) for x in lin(self.policy.student)], [host(x.bias) for x in lin(self.policy.student)], "elu", device=dev)
        self.teacher = MlpPolicy([host(x.weight) for x in lin(self.policy.teacher)], [host(x.bias) for x in lin(self.policy.teacher)], "elu", device=dev)
        self.cell_s = LstmCell.from_module(self.policy.memory_s.rnn, device=dev)
        self.cell_t = LstmCell.from_module(self.policy.memory_t.rnn, device=dev) if self.teacher_recurrent else None
        self.normalizer = None
        if teacher_obs_normalization:
            from .obsnorm import ObsNormalizer

            m = self.policy.teacher_obs_normalizer
            self.normalizer = ObsNormalizer(m._mean.shape[1], m.eps, max_rows=env.num_envs, device=dev)
        self.storage = RolloutStorage(env.num_envs, num_steps_per_env, sd, td, A, seed=seed, device=dev)
        self.std = self.policy.std.detach().clone()
        self.collector = RecurrentDistillCollector(env, self.student, self.teacher, self.storage, self.std, self.cell_s, self.cell_t, student_group=self.student_group,
                                                   teacher_group=self.teacher_group, normalizer=self.normalizer, use_graph=use_graph, clip_actions=clip_actions)
        self.batch = types.SimpleNamespace(observations=self.storage.observations, teacher_actions=self.collector.teacher_actions, dones=self.storage.dones,
                                           h0=self.collector.h0, c0=self.collector.c0)
        self.iteration = 0

    def inference_policy(self):
        """the student as `runner.get_inference_policy()` hands it out: the MLP kernel, or for a recurrent student the stateful callable with
        `reset(dones)` on a cell and a head of its own (playing does not disturb the collection's state or the captured loop's buffers); a
        snapshot of the student at the time of the call"""
        if not self.recurrent:
            return self.student
        from .distill_recurrent import RecurrentStudentInferencePolicy
        from .lstm import LstmCell

        from .policy import MlpPolicy

        if self.learner == "hip":
            self.alg.store_into(self.policy)
        lin = [x for x in self.policy.student if isinstance(x, nn.Linear)]
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        head = MlpPolicy([host(x.weight) for x in lin], [host(x.bias) for x in lin], "elu", device=str(self.device))  # (its own output buffer: any row count)
        return RecurrentStudentInferencePolicy(LstmCell.from_module(self.policy.memory_s.rnn, device=str(self.device)), head, self.student_group)

    def __repr__(self):
        return (f"DistillTrainer(learner={self.learner!r}, alg={type(self.alg).__name__}, num_envs={self.env.num_envs}, student<-{self.student_group!r}, "
                f"teacher<-{self.teacher_group!r}, iteration={self.iteration})")

    def load_state_dict(self, state_dict) -> bool:
        """`StudentTeacher.load_state_dict`, then everything that mirrors the module on the device: the HIP learner's master parameters, both
        inference images, the teacher's normaliser, the std tensor.  Returns whether this was a resume."""
        resumed = self.policy.load_state_dict(state_dict)
        if self.learner == "hip":
            self.alg.load_from(self.policy)
        self.student.load_linear_layers(self.policy.student)
        self.teacher.load_linear_layers(self.policy.teacher)
        if self.recurrent:
            self.cell_s.load_module(self.policy.memory_s.rnn)
            if self.cell_t is not None:
                self.cell_t.load_module(self.policy.memory_t.rnn)
        if self.normalizer is not None:
            self.normalizer.load_module(self.policy.teacher_obs_normalizer)
        self.std.copy_(self.policy.std.detach())
        return resumed

    def state_dict(self):
        if self.learner == "hip":
            self.alg.store_into(self.policy)
        return self.policy.state_dict()

    def _push(self):
        if self.recurrent:
            if self.learner == "hip":
                self.alg.push(self.cell_s, self.student)
            else:
                self.cell_s.load_module(self.policy.memory_s.rnn)
                self.student.load_linear_layers(self.policy.student)
            if self.carry_learner_state:  # what rsl_rl's `last_hidden_states` is believed to do; the reset mask of the next step 0 stays dones[T - 1]
                self.collector.set_student_state(*self.alg.final_state)
        elif self.learner == "hip":
            self.alg.push(self.student)  # device to device on the current stream; the next collection follows it on the same stream
        else:
            self.student.load_linear_layers(self.policy.student)

    def iterate(self) -> dict:
        if not self.policy.loaded_teacher:
            raise RuntimeError("DistillTrainer.iterate: no teacher is loaded (load_state_dict with a PPO checkpoint comes first)")
        self.collector.collect()
        st = self.storage
        out = dict(mean_reward=float(st.rewards.mean()), done_rate=float(st.dones.float().mean()))
        out.update(self.alg.update(self.batch))
        self._push()
        out["learning_rate"] = float(self.alg.learning_rate)
        out["grad_norm"] = float(self.alg.last_grad_norm)
        self.iteration += 1
        return out
