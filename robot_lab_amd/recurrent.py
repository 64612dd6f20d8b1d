"""THE RULE of recurrent policies: an LSTM in front of the actor's and the critic's MLP, what the reference's
`rsl_rl_recurrent_cfg_entry_point` tasks train (`RslRlRNNModelCfg(rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)` in front of a
128-128-128 ELU MLP, actor and critic alike).  rsl-rl-lib is third-party and not in the reference tree, so what follows is the
definition (INTEGRATION.md section 11 says where it knowingly differs from what rsl_rl 3.0.1 is believed to do); the device half
is csrc/rl_lstm.hip (include/rl_lstm.h) inside the captured collection loop (robot_lab_amd/collect.py).

Collection.  Step t of env e:  (h~, c~) = 0 if the PREVIOUS env.step of e set `done` (terminated or timed out) else (h, c);
(h', c') = LSTM(obs_t, (h~, c~)); mean_t = actor(h'_a), V_t = critic(h'_c).  (h~, c~) of both networks is saved with the transition:
the state the step saw.  No state crosses a done.
Bootstrap.  V(obs_T) of `compute_returns` is critic(LSTM_c(obs_T, (h~, c~))) from the current critic state; the state it produces is
NOT committed, so each observation enters the critic's memory once.
Update.  Mini-batches are contiguous blocks of N // num_mini_batches envs, in order, over all T steps (the remainder envs are left out, no
shuffle).  Per block the recurrence runs over t = 0 .. T - 1 from the SAVED state of step 0 (stale across the epochs: that is the
rule), the input state zeroed at every (row, step) that follows a done; everything after the networks is `PPO.minibatch_loss` /
`PPO.optimizer_step` over the T x block rows."""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from .ppo import PPO, mlp


class Memory(nn.Module):
    """rsl_rl's `Memory`: the `rnn` attribute is what names the checkpoint keys (`memory_a.rnn.weight_ih_l0`, ...)"""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.rnn = nn.LSTM(input_size, hidden_size, 1)

    def forward(self, x, h0, c0, reset=None):
        """The masked recurrence.  x [T, n, D]; (h0, c0) [n, H]: the state step 0 starts from (its own reset already applied);
        reset [T, n] bool or None: reset[t] zeroes the input state of step t (row 0 is not read).  Returns the outputs h'_t, [T, n, H],
        and the final (h, c).  The input half of the gates is one GEMM over all T n rows; the cell is nn.LSTM's (gates i, f, g, o)."""
        r = self.rnn
        zx = F.linear(x, r.weight_ih_l0, r.bias_ih_l0)
        h, c, out = h0, c0, []
        for t in range(x.shape[0]):
            if reset is not None and t > 0:
                keep = (~reset[t]).to(x.dtype).unsqueeze(-1)
                h, c = h * keep, c * keep
            i, f, g, o = (zx[t] + F.linear(h, r.weight_hh_l0, r.bias_hh_l0)).chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out.append(h)
        return torch.stack(out), (h, c)


class ActorCriticRecurrent(nn.Module):
    """rsl_rl `ActorCriticRecurrent`: `memory_a` / `memory_c` (a single-layer LSTM each) in front of the ELU MLPs `actor` / `critic` of input
    width `rnn_hidden_dim`, the scalar-type `std`.  `state_dict()` keys are rsl_rl's: `memory_a.rnn.weight_ih_l0`, `weight_hh_l0`, `bias_ih_l0`,
    `bias_hh_l0`, the same under `memory_c`, `actor.<2l>.*`, `critic.<2l>.*`, `std`."""
    is_recurrent = True

    def __init__(self, obs_dim, critic_obs_dim, act_dim, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128), init_noise_std=1.0,
                 rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1):
        super().__init__()
        check_rnn_cfg("ActorCriticRecurrent", rnn_type, rnn_hidden_dim, rnn_num_layers)
        self.rnn_hidden_dim = int(rnn_hidden_dim)
        self.memory_a = Memory(obs_dim, self.rnn_hidden_dim)
        self.memory_c = Memory(critic_obs_dim, self.rnn_hidden_dim)
        self.actor = mlp([self.rnn_hidden_dim, *actor_hidden, act_dim])
        self.critic = mlp([self.rnn_hidden_dim, *critic_hidden, 1])
        self.std = nn.Parameter(init_noise_std * torch.ones(act_dim))

    def unroll(self, obs, critic_obs, hidden_a, hidden_c, reset=None):
        """(mean [T, n, A], value [T, n]) of a block of trajectories: see `Memory.forward`"""
        ha, _ = self.memory_a(obs, *hidden_a, reset)
        hc, _ = self.memory_c(critic_obs, *hidden_c, reset)
        return self.actor(ha), self.critic(hc).squeeze(-1)


def check_rnn_cfg(who, rnn_type, rnn_hidden_dim, rnn_num_layers):
    """what of rsl_rl's rnn settings is implemented; the rest is refused with a reason, never ignored"""
    if rnn_type == "gru":
        raise NotImplementedError(f"{who}: rnn_type=\"gru\" is not implemented: the device cell (csrc/rl_lstm.hip) and the rule (robot_lab_amd/recurrent.py) "
                                  "are the LSTM's, which is what every recurrent agent cfg of the reference uses; use rnn_type=\"lstm\"")
    if rnn_type != "lstm":
        raise ValueError(f"{who}: rnn_type must be \"lstm\", not {rnn_type!r}")
    if int(rnn_num_layers) != 1:
        raise NotImplementedError(f"{who}: rnn_num_layers={rnn_num_layers} is not implemented: the collection step runs ONE cell per network and the saved "
                                  "state is one (h, c) pair per transition; use rnn_num_layers=1 (the reference's recurrent cfgs do)")
    if not 1 <= int(rnn_hidden_dim) <= 512:
        raise ValueError(f"{who}: rnn_hidden_dim={rnn_hidden_dim} is outside 1..512, what the cell kernel and the MLP heads take as a row width")


class RecurrentBatch:
    """A filled `RolloutStorage` plus the saved states of step 0 - `hidden_a` = (h, c) of the actor's memory, `hidden_c` of the critic's, each
    [N, H] - as `RecurrentPPO.update` reads them; every other attribute is the storage's."""

    def __init__(self, storage, hidden_a, hidden_c):
        self._storage, self.hidden_a, self.hidden_c = storage, hidden_a, hidden_c

    def __getattr__(self, name):
        return getattr(self._storage, name)


class RecurrentPPO(PPO):
    """`PPO` on an `ActorCriticRecurrent`: the update of the module docstring.  Everything behind the networks' outputs is `PPO`'s own code."""

    def __init__(self, policy, **kw):
        for refused, why in (("symmetry", "mirroring an observation sequence through the memory is not defined here"),
                             ("mirror_loss", "it needs symmetry="), ("group", "the ranks' block order and state exchange are not decided")):
            v = kw.get(refused)
            if v is not None and not (refused == "group" and getattr(v, "world_size", 1) <= 1):
                raise NotImplementedError(f"RecurrentPPO: {refused}= with a recurrent policy is not implemented: {why}")
        if not isinstance(policy, ActorCriticRecurrent):
            raise TypeError(f"RecurrentPPO: policy must be an ActorCriticRecurrent, not {type(policy).__name__}")
        super().__init__(policy, **kw)

    def blocks(self, num_envs):
        """[(first env, one past the last)] of the mini-batches: contiguous, in order, N // num_mini_batches envs each; the remainder is left out"""
        n = num_envs // self.num_mini_batches
        if n < 1:
            raise ValueError(f"RecurrentPPO: {num_envs} envs do not fill {self.num_mini_batches} mini-batches of whole trajectories")
        return [(i * n, (i + 1) * n) for i in range(self.num_mini_batches)]

    def block_loss(self, batch, lo, hi, stats):
        """the loss of the mini-batch of envs lo .. hi - 1 over all T steps, rows in [T, block] order"""
        sl = slice(lo, hi)
        dones = batch.dones[:, sl].to(torch.bool)
        reset = torch.cat([torch.zeros_like(dones[:1]), dones[:-1]], 0)  # the input state of step t is zeroed where step t - 1 ended an episode
        mean, value = self.policy.unroll(batch.observations[:, sl], batch.privileged_observations[:, sl], tuple(t[sl] for t in batch.hidden_a),
                                         tuple(t[sl] for t in batch.hidden_c), reset)
        flat = lambda t: t[:, sl].reshape(-1, *t.shape[2:])  # noqa: E731
        mean = mean.reshape(-1, mean.shape[-1])
        n = mean.shape[0]
        return self.minibatch_loss(stats, flat(batch.actions), mean, self.policy.std.expand_as(mean), value.reshape(-1), n, flat(batch.actions_log_prob).view(-1),
                                   flat(batch.advantages).view(-1), flat(batch.values).view(-1), flat(batch.returns).view(-1), flat(batch.mu), flat(batch.sigma))

    def update(self, batch, generator=None) -> dict:
        """`batch`: a `RecurrentBatch`.  `generator` is not drawn from: there is no shuffle."""
        stats = dict(value_loss=0.0, surrogate_loss=0.0, entropy=0.0, kl=0.0)
        n_updates = 0
        for _ in range(self.num_learning_epochs):
            for lo, hi in self.blocks(batch.num_envs):
                self.optimizer_step(self.block_loss(batch, lo, hi, stats))
                n_updates += 1
        out = {k: v / max(n_updates, 1) for k, v in stats.items()}
        out["learning_rate"] = self.learning_rate
        return out


def read_recurrent_cfg(train_cfg: dict):
    """The `Trainer` keywords of a recurrent runner cfg, or None when the cfg is feed-forward.  Pure (no device, no env).  Two spellings:
      - rsl_rl 3.0.1's: policy = dict(class_name="ActorCriticRecurrent", actor_hidden_dims, critic_hidden_dims, init_noise_std, rnn_type,
        rnn_hidden_dim, rnn_num_layers);
      - the reference's: `actor=` / `critic=` model cfgs with class_name="RNNModel" (RslRlRNNModelCfg: hidden_dims, activation, rnn_type,
        rnn_hidden_dim, rnn_num_layers, distribution_cfg.init_std), equal rnn settings in both.
    `obs_groups` {"actor": ["policy"], "critic": ["policy"]} makes the critic read the policy group (`critic_group="policy"`).
    What is not implemented is refused with a reason."""
    from dataclasses import MISSING

    given = lambda d, k, default=None: default if d.get(k, default) is None or d.get(k, default) is MISSING else d.get(k, default)  # noqa: E731
    pol = given(train_cfg, "policy", {}) or {}
    actor, critic = given(train_cfg, "actor"), given(train_cfg, "critic")
    models = isinstance(actor, dict) and isinstance(critic, dict) and (actor.get("class_name") == "RNNModel" or critic.get("class_name") == "RNNModel"
                                                                      or given(actor, "rnn_type") is not None or given(critic, "rnn_type") is not None)
    if models:
        if pol:
            raise ValueError("stand-in runner: the cfg has both `policy=` and `actor=` / `critic=` model cfgs: give one spelling")
        for role, m in (("actor", actor), ("critic", critic)):
            if m.get("class_name", "RNNModel") != "RNNModel" or given(m, "rnn_type") is None:
                raise NotImplementedError(f"stand-in runner: the {role} is {m.get('class_name')!r} (rnn_type={m.get('rnn_type')!r}) while the other network is "
                                          "recurrent: a recurrent actor with a feed-forward critic (or the reverse) is not implemented - both are RNNModel")
            if given(m, "activation", "elu") != "elu":
                raise NotImplementedError(f"stand-in runner: {role} activation={m.get('activation')!r}; ELU networks only")
            if given(m, "obs_normalization", False):
                raise NotImplementedError(f"stand-in runner: {role} obs_normalization=True with a recurrent model is not implemented (recurrence together with "
                                          "observation normalisation is a follow-up); set it to False")
            if given(m, "hidden_dims") is None:
                raise ValueError(f"stand-in runner: the {role} model cfg has no hidden_dims")
        rnn = tuple((given(m, "rnn_type"), int(given(m, "rnn_hidden_dim", 256)), int(given(m, "rnn_num_layers", 1))) for m in (actor, critic))
        if rnn[0] != rnn[1]:
            raise NotImplementedError(f"stand-in runner: actor and critic rnn settings differ ({rnn[0]} / {rnn[1]}): ActorCriticRecurrent has one "
                                      "rnn_type / rnn_hidden_dim / rnn_num_layers for both memories")
        dist = given(actor, "distribution_cfg", {}) or {}
        kw = dict(actor_hidden=tuple(actor["hidden_dims"]), critic_hidden=tuple(critic["hidden_dims"]), init_noise_std=float(given(dist, "init_std", 1.0)),
                  rnn_type=rnn[0][0], rnn_hidden_dim=rnn[0][1], rnn_num_layers=rnn[0][2])
    elif pol.get("class_name") == "ActorCriticRecurrent" or given(pol, "rnn_type") is not None:
        if pol.get("class_name", "ActorCriticRecurrent") != "ActorCriticRecurrent":
            raise NotImplementedError(f"stand-in runner: policy.class_name={pol.get('class_name')!r} with rnn_type={pol.get('rnn_type')!r}: a recurrent policy is "
                                      "class_name=\"ActorCriticRecurrent\"")
        if given(pol, "activation", "elu") != "elu":
            raise NotImplementedError("stand-in runner: ELU networks only (what every robot_lab agent cfg uses)")
        if pol.get("actor_obs_normalization") or pol.get("critic_obs_normalization"):
            raise NotImplementedError("stand-in runner: observation normalisation with a recurrent policy is not implemented (a follow-up); drop the "
                                      "*_obs_normalization flags")
        kw = dict(actor_hidden=tuple(given(pol, "actor_hidden_dims", (128, 128, 128))), critic_hidden=tuple(given(pol, "critic_hidden_dims", (128, 128, 128))),
                  init_noise_std=float(given(pol, "init_noise_std", 1.0)), rnn_type=given(pol, "rnn_type", "lstm"),
                  rnn_hidden_dim=int(given(pol, "rnn_hidden_dim", 256)), rnn_num_layers=int(given(pol, "rnn_num_layers", 1)))
    else:
        return None
    check_rnn_cfg("stand-in runner", kw["rnn_type"], kw["rnn_hidden_dim"], kw["rnn_num_layers"])
    groups = dict(given(train_cfg, "obs_groups", {}) or {})
    actor_set = list(groups.get("policy", groups.get("actor", ["policy"])))
    critic_set = list(groups.get("critic", ["critic"]))
    if actor_set != ["policy"] or critic_set not in (["critic"], ["policy"]):
        raise NotImplementedError(f"stand-in runner: obs_groups {groups} - a recurrent policy reads actor <- ['policy'] and critic <- ['critic'] or ['policy']; "
                                  "exactly one observation group per network is wired to the cell kernel (no concatenation of groups)")
    kw["critic_group"] = critic_set[0]
    return kw


class RecurrentInferencePolicy:
    """`runner.get_inference_policy()` of a recurrent policy: a stateful callable - `policy(obs)` advances the actor's memory by one step on the
    cell kernel and returns the actor MLP's mean, `policy.reset(dones)` zeroes the state of the rows with `dones` before their next step
    (`reset()` / `reset(None)`: every row), which is what play.py:246 calls after `env.step`."""

    def __init__(self, cell, actor):
        self.cell, self.actor = cell, actor
        self._h = self._c = self._mask = None
        self._k = 0

    def _alloc(self, n):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=self.cell.device)  # noqa: E731
        H = self.cell.hidden
        self._h, self._c, self._mask, self._k = (z(n, H), z(n, H)), (z(n, H), z(n, H)), z(n, dt=torch.uint8), 0

    def reset(self, dones=None):
        if self._mask is None:
            return
        if dones is None:
            self._mask.fill_(1)
        else:
            self._mask |= dones.to(device=self._mask.device).reshape(-1).to(torch.uint8).ne(0).to(torch.uint8)

    @torch.inference_mode()
    def __call__(self, obs):
        obs = obs if torch.is_tensor(obs) else obs["policy"]
        obs = obs.to(device=self.cell.device, dtype=torch.float32).contiguous()
        if self._mask is None or self._mask.numel() != obs.shape[0]:
            self._alloc(obs.shape[0])
        k = self._k
        self.cell.step(obs, self._h[k], self._c[k], self._h[1 - k], self._c[1 - k], reset=self._mask)
        self._mask.zero_()
        self._k = 1 - k
        return self.actor(self._h[1 - k])
