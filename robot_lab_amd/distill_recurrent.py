"""THE RULE of recurrent distillation: an LSTM in front of the student's MLP (and, usually, of the teacher's), what the reference's
`rsl_rl_distillation_recurrent_cfg_entry_point` trains (`AnymalDFlatDistillationRunnerRecurrentCfg`: `RslRlRNNModelCfg(rnn_type="lstm",
rnn_hidden_dim=256, rnn_num_layers=1)` in front of a 128-128-128 ELU MLP, student and teacher alike).  rsl-rl-lib is not in the reference tree,
so what follows is the definition, as `distill.py` is for a feed-forward student and `recurrent.py` for recurrent PPO; the HIP learner is
robot_lab_amd/distill_recurrent_hip.py (include/rl_distill_bptt.h).

    policy = StudentTeacherRecurrent(obs_dim, teacher_obs_dim, act_dim, student_hidden, teacher_hidden, init_noise_std, rnn_hidden_dim=256)
    policy.load_state_dict(torch.load(teacher_checkpoint)["model_state_dict"])   # a recurrent PPO checkpoint: memory_a, actor -> the teacher
    alg = RecurrentDistillation(policy, num_learning_epochs=2, gradient_length=15, learning_rate=1e-3)
    alg.update(batch)     # observations [T, N, obs], teacher_actions [T, N, A], dones [T, N], h0, c0 [N, H] -> {"behavior": mean loss}
    alg.final_state       # (h, c) after step T - 1 of the last epoch

The update (truncated back-propagation through time over groups of `gradient_length` steps):

    cnt = 0; loss = 0; total = 0
    for each epoch:
        (h, c) = (h0, c0), no gradient            # every epoch restarts from the saved state
        for t in 0 .. T-1:
            if t >= 1: (h, c) = 0 where dones[t-1]   # a select; no gradient crosses a done
            (h, c) = LSTM(obs[t], (h, c)); l_t = loss_fn(student(h), teacher_actions[t])   # mean over N*A
            loss += l_t; total += float(l_t); cnt += 1
            if cnt % gradient_length == 0:
                backward(loss); clip; Adam; loss = 0
                detach (h, c)                        # the carried VALUES were computed with the weights from before this step
    return {"behavior": total / cnt}; final_state = (h, c) after step T-1 of the last epoch, dones[T-1] not applied

What follows from it:
  - `cnt` runs across the epochs, as in `Distillation.update`: a group may contain one or several epoch boundaries (`gradient_length > T`).
  - Gradient does not flow from a step to its predecessor when the predecessor ended an episode, when the predecessor belongs to an earlier
    group, or when the step is t = 0 of an epoch, whose state is `h0` / `c0`.
  - Left-over steps get a forward and the head for the statistic only.
  - `dones[T - 1]` is never read by the update.
  - `bias_ih` and `bias_hh` are two parameters with equal gradients and their own Adam moments.
  - The teacher is not evaluated in the update: its actions were stored at collection."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from .distill import behavior_loss
from .ppo import EmpiricalNormalization, mlp
from .recurrent import Memory, RecurrentInferencePolicy, check_rnn_cfg

LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def lstm_step(rnn, x, h, c):
    """one step of a single-layer nn.LSTM (gates i, f, g, o) written out, as `Memory.forward` has it"""
    i, f, g, o = (F.linear(x, rnn.weight_ih_l0, rnn.bias_ih_l0) + F.linear(h, rnn.weight_hh_l0, rnn.bias_hh_l0)).chunk(4, -1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


class StudentTeacherRecurrent(nn.Module):
    """rsl_rl 3.0.1 `StudentTeacherRecurrent` for a single-layer LSTM and ELU networks: `memory_s` in front of `student`; with
    `teacher_recurrent` `memory_t` in front of `teacher`, without it the feed-forward teacher of `distill.StudentTeacher`.  `state_dict()` keys
    are rsl_rl's: `memory_s.rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l0`, the same under `memory_t`, `student.*`, `teacher.*`, `std`,
    `teacher_obs_normalizer.*`.  The teacher is in eval mode and never differentiated; `std` is not trained."""
    is_recurrent = True

    def __init__(self, obs_dim, teacher_obs_dim, act_dim, student_hidden=(128, 128, 128), teacher_hidden=(128, 128, 128), init_noise_std=0.1,
                 rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1, teacher_recurrent=True, teacher_obs_normalization=False):
        super().__init__()
        check_rnn_cfg("StudentTeacherRecurrent", rnn_type, rnn_hidden_dim, rnn_num_layers)
        H = self.rnn_hidden_dim = int(rnn_hidden_dim)
        self.teacher_recurrent = bool(teacher_recurrent)
        self.loaded_teacher = False
        self.memory_s = Memory(obs_dim, H)
        self.student = mlp([H, *student_hidden, act_dim])
        if self.teacher_recurrent:
            self.memory_t = Memory(teacher_obs_dim, H)
        self.teacher = mlp([H if self.teacher_recurrent else teacher_obs_dim, *teacher_hidden, act_dim])
        self.std = nn.Parameter(init_noise_std * torch.ones(act_dim))
        self.teacher_obs_normalization = bool(teacher_obs_normalization)
        if teacher_obs_normalization:
            self.teacher_obs_normalizer = EmpiricalNormalization(teacher_obs_dim)
        else:
            self.teacher_obs_normalizer = nn.Identity()
        for p in self._teacher_parameters():
            p.requires_grad_(False)
        self.train(self.training)

    def _teacher_parameters(self):
        return list(self.memory_t.parameters() if self.teacher_recurrent else []) + list(self.teacher.parameters())

    def trained_parameters(self):
        """what receives a gradient, in the flat order of the HIP learner and the parameter order of the optimiser: the student's memory, then its MLP"""
        return list(self.memory_s.parameters()) + list(self.student.parameters())

    def train(self, mode=True):
        super().train(mode)
        self.teacher.eval()
        self.teacher_obs_normalizer.eval()
        if self.teacher_recurrent:
            self.memory_t.eval()
        return self

    def load_state_dict(self, state_dict, strict=True):
        """A recurrent PPO checkpoint (`memory_a.rnn.*` present) becomes a recurrent teacher: `memory_a.rnn.*` -> `memory_t.rnn.*`, `actor.*` ->
        `teacher.*`, strict on names and shapes; returns False.  A feed-forward PPO checkpoint (`actor.*` without a memory) becomes a
        feed-forward teacher; returns False.  A PPO checkpoint whose kind does not match `teacher_recurrent` is an error that names the keyword.
        A distillation checkpoint (`student.*` and `memory_s.*`) is loaded strictly; returns True.  Anything else is an error."""
        keys = list(state_dict.keys())
        who = "StudentTeacherRecurrent.load_state_dict"
        if any(k.startswith("actor.") for k in keys):
            recurrent = any(k.startswith("memory_a.") for k in keys)
            if recurrent != self.teacher_recurrent:
                raise RuntimeError(f"{who}: the PPO checkpoint is " + ("recurrent (memory_a.rnn.* present)" if recurrent else "feed-forward (no memory_a.rnn.*)") +
                                   f" but this policy was built with teacher_recurrent={self.teacher_recurrent}: build it with teacher_recurrent={recurrent}")
            norm = {k[len("actor_obs_normalizer."):]: v for k, v in state_dict.items() if k.startswith("actor_obs_normalizer.")}
            if bool(norm) != self.teacher_obs_normalization:
                raise RuntimeError(f"{who}: the PPO checkpoint " + ("carries" if norm else "has no") + " actor_obs_normalizer.* but this policy was built with "
                                   f"teacher_obs_normalization={self.teacher_obs_normalization}: the teacher would see rows it was not trained on (build the "
                                   f"policy with teacher_obs_normalization={bool(norm)})")
            self.teacher.load_state_dict({k[len("actor."):]: v for k, v in state_dict.items() if k.startswith("actor.")}, strict=True)
            if recurrent:
                self.memory_t.load_state_dict({k[len("memory_a."):]: v for k, v in state_dict.items() if k.startswith("memory_a.")}, strict=True)
            if norm:
                self.teacher_obs_normalizer.load_state_dict(norm, strict=True)
            self.loaded_teacher = True
            self.train(self.training)
            return False
        if any(k.startswith("student.") for k in keys):
            if not any(k.startswith("memory_s.") for k in keys):
                raise RuntimeError(f"{who}: the distillation checkpoint has student.* but no memory_s.rnn.*: it holds a feed-forward student "
                                   "(load it into distill.StudentTeacher; DistillTrainer without rnn_type=)")
            recurrent = any(k.startswith("memory_t.") for k in keys)
            if recurrent != self.teacher_recurrent:
                raise RuntimeError(f"{who}: the distillation checkpoint has " + ("a recurrent teacher (memory_t.rnn.*)" if recurrent else "a feed-forward teacher (no memory_t.rnn.*)") +
                                   f" but this policy was built with teacher_recurrent={self.teacher_recurrent}: build it with teacher_recurrent={recurrent}")
            super().load_state_dict(state_dict, strict=True)
            self.loaded_teacher = True
            self.train(self.training)
            return True
        raise ValueError(f"{who}: the state dict has neither actor.* (a PPO checkpoint, which becomes the teacher) nor student.* (a distillation "
                         f"checkpoint) keys: {keys[:6]}")


class RecurrentDistillation:
    """The update of the module docstring on a `StudentTeacherRecurrent`.  `batch`: `observations` [T, N, obs], `teacher_actions` [T, N, A],
    `dones` [T, N], `h0`, `c0` [N, H] - the student state step 0 of the collection saw, with its own reset already applied.  Afterwards
    `final_state` is (h, c) behind step T - 1 of the last epoch (dones[T - 1] not applied)."""

    def __init__(self, policy: StudentTeacherRecurrent, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse"):
        if not isinstance(policy, StudentTeacherRecurrent):
            raise TypeError(f"RecurrentDistillation: policy must be a StudentTeacherRecurrent, not {type(policy).__name__}")
        if num_learning_epochs < 1 or gradient_length < 1:
            raise ValueError("RecurrentDistillation: num_learning_epochs and gradient_length must be >= 1")
        self.policy = policy
        self.num_learning_epochs, self.gradient_length, self.learning_rate, self.max_grad_norm = num_learning_epochs, gradient_length, learning_rate, max_grad_norm
        self.loss_type, self.loss_fn = loss_type, behavior_loss(loss_type)
        self.optimizer = torch.optim.Adam(policy.trained_parameters(), lr=learning_rate)
        self.last_grad_norm = float("nan")
        self.grad_norms = []  # the pre-clip gradient norms of the last update, one per optimiser step
        self.num_updates = 0
        self.final_state = None
        self.on_backward = None  # (for tests) called with the group's number after its backward, before clip and Adam

    def update(self, batch) -> dict:
        obs, teacher_actions = batch.observations, batch.teacher_actions
        dones = batch.dones.to(torch.bool)
        rnn, student, params = self.policy.memory_s.rnn, self.policy.student, self.policy.trained_parameters()
        self.grad_norms = []
        cnt, loss, total = 0, 0, 0.0
        for _ in range(self.num_learning_epochs):
            h, c = batch.h0.detach(), batch.c0.detach()
            for t in range(obs.shape[0]):
                if t >= 1:
                    gone = dones[t - 1].unsqueeze(-1)
                    h, c = torch.where(gone, torch.zeros_like(h), h), torch.where(gone, torch.zeros_like(c), c)
                h, c = lstm_step(rnn, obs[t], h, c)
                l_t = self.loss_fn(student(h), teacher_actions[t])  # the mean over the N * act_dim entries
                loss = loss + l_t
                total += float(l_t.detach())
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    if self.on_backward is not None:
                        self.on_backward(cnt // self.gradient_length - 1)
                    norm = nn.utils.clip_grad_norm_(params, self.max_grad_norm if self.max_grad_norm else float("inf"))
                    self.last_grad_norm = float(norm)
                    self.grad_norms.append(self.last_grad_norm)
                    self.optimizer.step()
                    self.num_updates += 1
                    loss = 0
                    h, c = h.detach(), c.detach()
        self.final_state = (h.detach(), c.detach())
        return {"behavior": total / cnt}


def trained_shapes(obs_dim, hidden, head_dims):
    """shapes of `StudentTeacherRecurrent.trained_parameters()` (= the flat layout of include/rl_distill_bptt.h): weight_ih, weight_hh, bias_ih,
    bias_hh of memory_s; W, b per student layer"""
    H4 = 4 * hidden
    return [(H4, obs_dim), (H4, hidden), (H4,), (H4,)] + [s for l in range(len(head_dims) - 1) for s in ((head_dims[l + 1], head_dims[l]), (head_dims[l + 1],))]


class RecurrentStudentInferencePolicy(RecurrentInferencePolicy):
    """`runner.get_inference_policy()` of a recurrent student: `policy(obs)` advances the student's memory by one step on the cell kernel and
    returns the student MLP's mean, `policy.reset(dones)` zeroes the state of the rows with `dones` before their next step."""

    def __init__(self, cell, student, group="policy"):
        super().__init__(cell, student)
        self.group = group

    def __call__(self, obs):
        return super().__call__(obs if torch.is_tensor(obs) else obs[self.group])
