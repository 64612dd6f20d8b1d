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
the eager loop bit for bit (tests/test_gpu_distill.py)."""
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
