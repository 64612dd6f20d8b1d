"""The data-collection half of a distillation iteration as ONE hipGraph launch: `Collector` (robot_lab_amd/collect.py) for rsl_rl's
`Distillation.act` / `process_env_step`.  Existing kernels only.  Per step

    student and teacher in ONE launch (rl_mlp_forward_pair): the teacher's [N, act_dim] output goes straight into slot t of the
    [T, N, act_dim] tensor this collector owns (`teacher_actions`) - the launch takes the second network's output address
    -> the sampling head (rl_rollout_act: a = mu + std z on this library's Philox stream; the UNFUSED route - the fused act epilogue hands the
    second network's output address to the storage's values slot, one float per env, which a teacher of act_dim outputs would overrun)
    -> env.step(actions, rollout=storage)

The `RolloutStorage` holds the student's rows (observations), the teacher's rows (its critic slot, RAW), actions, rewards and dones; its value
slot is zero, so the env kernel's time-out bootstrap adds nothing.  With a `normalizer` (the teacher's `actor_obs_normalizer` of its PPO run) one
`apply` runs in front of the teacher; the statistics are never updated.  Captured under `Collector`'s conditions (T even); a replay equals
the eager loop bit for bit (tests/test_gpu_distill.py).

`RecurrentDistillCollector` is the same loop for a recurrent student (robot_lab_amd/distill_recurrent.py): two memories in front of the two MLPs,
ONE `rl_lstm_step_pair` per step for the student's and the teacher's cell (one `rl_lstm_step` for the student with a feed-forward teacher), the
reset mask the done bytes of storage slot t - 1, and only step 0 saves the student's (h~, c~): the update's `h0` / `c0`."""
from __future__ import annotations

import torch


class DistillCollector:
    def __init__(self, env, student, teacher, storage, action_std: torch.Tensor, student_group: str = "policy", teacher_group: str = "policy", normalizer=None,
                 use_graph: bool = True, clip_actions: float | None = None, gamma: float = 0.99):
        self.env, self.student, self.teacher, self.storage = env, student, teacher, storage
        self.std, self.student_group, self.teacher_group, self.normalizer = action_std, student_group, teacher_group, normalizer
        self.clip_actions, self.gamma = clip_actions, gamma
        self.T = storage.num_transitions_per_env
        self.obs = env.get_observations()
        for g in (student_group, teacher_group):
            if g not in self.obs:
                raise ValueError(f"DistillCollector: observation group {g!r} is not one of the env's ({sorted(self.obs.keys())})")
        N, dev = env.num_envs, storage.device
        self.teacher_actions = torch.zeros(self.T, N, teacher.out_dim, device=dev, dtype=torch.float32)
        self._zero_values = torch.zeros(N, device=dev, dtype=torch.float32)
        self._norm_rows = torch.empty_like(self.obs[teacher_group]) if normalizer is not None else None
        if self.T % 2:
            use_graph = False  # the env's observation buffers alternate: a captured loop needs an even number of steps
        self.use_graph = use_graph
        self._graph, self._warm = None, False

    def _iteration(self, obs):
        st, env = self.storage, self.env
        st.clear()
        for t in range(self.T):
            s_rows, t_rows = obs[self.student_group], obs[self.teacher_group]
            seen = t_rows if self.normalizer is None else self.normalizer.apply(t_rows, out=self._norm_rows)
            mean, _ = self.student.forward_pair(s_rows, self.teacher, seen, other_out=self.teacher_actions[t])
            actions = st.act(s_rows, t_rows, mean, self.std, self._zero_values)
            if self.clip_actions is not None:
                actions = actions.clamp(-self.clip_actions, self.clip_actions)
            obs, _, _, _, _ = env.step(actions, rollout=st, gamma=self.gamma)
        return obs

    def _capture(self):
        env, st = self.env, self.storage
        g = torch.cuda.CUDAGraph()
        env.graph_begin()
        st.graph_begin()
        start = self.obs
        with torch.cuda.graph(g):
            end = self._iteration(start)
            n_env, n_ro = env.graph_end(), st.graph_end()
        assert n_env == self.T and n_ro == self.T, (n_env, n_ro)
        assert end[self.student_group].data_ptr() == start[self.student_group].data_ptr()
        self._graph = g

    @torch.inference_mode()
    def collect(self):
        """One iteration: fills the storage and `teacher_actions`, returns the observations of the next one."""
        if not self.use_graph:
            self.obs = self._iteration(self.obs)
            return self.obs
        if not self._warm:  # eager once: every library has its per-device setup behind it
            self._warm = True
            self.obs = self._iteration(self.obs)
            return self.obs
        if self._graph is None:
            self._capture()
        self.env.graph_launching(self.T)
        self.storage.graph_launching()
        self._graph.replay()
        self.obs = self.env.get_observations()
        return self.obs


class RecurrentDistillCollector(DistillCollector):
    """`DistillCollector` with memories (csrc/rl_lstm.hip, robot_lab_amd/lstm.py `LstmCell`): `cell_s` in front of `student`, `cell_t` in front of
    `teacher` or None for a feed-forward teacher, which reads its raw (optionally normalised) rows as before.  Per step: the cell launch - the reset of
    the previous step's dones applied, read from storage slot t - 1 without a launch of their own (step 0 reads `reset`, which takes the last slot
    once per iteration) -, the two MLPs in one launch on the student's h' and the teacher's h' (or rows), the unfused act, env.step.  `h0` / `c0`
    [N, H]: the student state step 0 saw, its own reset applied.  The state lives in two ping-pong buffers; T even brings a captured loop back to
    the buffers it started from."""

    def __init__(self, env, student, teacher, storage, action_std, cell_s, cell_t=None, **kw):
        super().__init__(env, student, teacher, storage, action_std, **kw)
        N, dev, H = env.num_envs, storage.device, cell_s.hidden
        if student.in_dim != H or (cell_t is not None and teacher.in_dim != cell_t.hidden):
            raise ValueError(f"RecurrentDistillCollector: the MLPs read rows of {student.in_dim} / {teacher.in_dim} columns, the memories produce {H}" +
                             (f" / {cell_t.hidden}" if cell_t is not None else ""))
        self.cell_s, self.cell_t = cell_s, cell_t
        z = lambda n: torch.zeros(N, n, device=dev, dtype=torch.float32)  # noqa: E731
        self._hs, self._cs = (z(H), z(H)), (z(H), z(H))
        if cell_t is not None:
            self._ht, self._ct = (z(cell_t.hidden), z(cell_t.hidden)), (z(cell_t.hidden), z(cell_t.hidden))
        self._k = 0  # which of the two buffers holds the current state
        self.h0, self.c0 = z(H), z(H)
        self.reset = torch.zeros(N, dtype=torch.uint8, device=dev)

    def student_state(self):
        """(h, c) of the student as the next step will read them (before its reset)"""
        return self._hs[self._k], self._cs[self._k]

    def set_student_state(self, h, c):
        """the learner's final state becomes the collection's (stream-ordered copies into the buffers the next step reads)"""
        self._hs[self._k].copy_(h)
        self._cs[self._k].copy_(c)

    def _iteration(self, obs):
        st, env = self.storage, self.env
        st.clear()
        dones = st.dones.view(torch.uint8)
        for t in range(self.T):
            s_rows, t_rows = obs[self.student_group], obs[self.teacher_group]
            seen = t_rows if self.normalizer is None else self.normalizer.apply(t_rows, out=self._norm_rows)
            k = self._k
            reset = self.reset if t == 0 else dones[t - 1]
            saved = dict(h_saved=self.h0, c_saved=self.c0) if t == 0 else {}
            if self.cell_t is not None:
                self.cell_s.step_pair(s_rows, self._hs[k], self._cs[k], self._hs[1 - k], self._cs[1 - k], self.cell_t, seen, self._ht[k], self._ct[k],
                                      self._ht[1 - k], self._ct[1 - k], reset=reset, **saved)
                seen = self._ht[1 - k]
            else:
                self.cell_s.step(s_rows, self._hs[k], self._cs[k], self._hs[1 - k], self._cs[1 - k], reset=reset, **saved)
            self._k = 1 - k
            mean, _ = self.student.forward_pair(self._hs[1 - k], self.teacher, seen, other_out=self.teacher_actions[t])
            actions = st.act(s_rows, t_rows, mean, self.std, self._zero_values)
            if self.clip_actions is not None:
                actions = actions.clamp(-self.clip_actions, self.clip_actions)
            obs, _, _, _, _ = env.step(actions, rollout=st, gamma=self.gamma)
        self.reset.copy_(dones[self.T - 1])
        return obs
