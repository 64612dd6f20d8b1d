"""The learner half of a PPO iteration, so that a policy can actually be TRAINED on this env without the (absent) rsl-rl-lib:

    collect (HIP: csrc/rl_env.hip + rl_policy.hip + rl_rollout.hip, one hipGraph launch per iteration - robot_lab_amd/collect.py)
    -> update (this file: torch autograd on the stored batch) -> push the new parameters into the inference kernels in place
    (rl_mlp_set_weights) -> collect ...

What the reference gets from `runner.learn(...)` (scripts/reinforcement_learning/rsl_rl/train.py:224 -> rsl_rl `OnPolicyRunner.learn`
-> `PPO.update`), with the hyper-parameters of `.../unitree_a1/agents/rsl_rl_ppo_cfg.py:10-37`.  rsl-rl-lib (3.0.1) is third-party
and not in the reference tree: this restates its published update rule - clipped surrogate, clipped value loss, entropy bonus,
KL-adaptive learning rate, gradient-norm clipping, 5 epochs x 4 mini-batches over the T x N transitions - and is NOT pinned to the
library (no copy of it exists here); `tests/test_ppo.py` checks the pieces against their definitions.  The update is plain PyTorch
(autograd + rocBLAS / hipBLASLt GEMMs): it is off the env-step path this repository is about, host-side plumbing like the launcher,
and it is what makes `tools/train_demo.py` - the end-to-end check that the simulator is a learnable environment - possible."""
from __future__ import annotations

import functools
import math
import numbers

import torch
from torch import nn


def mlp(dims, activation=nn.ELU):
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            layers.append(activation())
    return nn.Sequential(*layers)


class EmpiricalNormalization(nn.Module):
    """THE RULE of the observation normalisation (rsl_rl `EmpiricalNormalization`): running mean and POPULATION variance of the rows it
    is shown, `forward(x) = (x - _mean) / (_std + eps)`.  The device half is csrc/rl_obsnorm.hip (include/rl_obsnorm.h), checked against
    this module; buffer names and shapes are rsl_rl's, so `state_dict()` keys are `<name>._mean`, `._var`, `._std`, `.count`."""

    def __init__(self, dim, eps=1e-2):
        super().__init__()
        self.eps = eps
        self.register_buffer("_mean", torch.zeros(1, dim))
        self.register_buffer("_var", torch.ones(1, dim))
        self.register_buffer("_std", torch.ones(1, dim))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        return (x - self._mean) / (self._std + self.eps)

    @torch.no_grad()
    def update(self, x):
        """Chan's merge of the state with the batch `x` [n, dim]; nothing happens outside training mode."""
        if not self.training:
            return
        n = x.shape[0]
        self.count += n
        rate = torch.tensor(n, dtype=torch.float32) / self.count.to(torch.float32)  # one fp32 division
        rate = rate.to(device=self._mean.device, dtype=self._mean.dtype)
        var_x, mean_x = torch.var_mean(x, dim=0, unbiased=False, keepdim=True)
        delta = mean_x - self._mean
        self._mean += rate * delta
        self._var += rate * (var_x - self._var + delta * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)


class ActorCritic(nn.Module):
    """rsl_rl `ActorCritic` as the cfg builds it (rsl_rl_ppo_cfg.py:15-22): two ELU MLPs, a state-independent standard deviation
    (`noise_std_type="scalar"`, init 1.0).  `state_dict()` keys follow rsl_rl (`actor.<2l>.weight`, `critic.<2l>.weight`, `std`), so
    checkpoints load into `robot_lab_amd.policy.MlpPolicy.from_state_dict` and the shim's exporters.
    `actor_obs_normalization` / `critic_obs_normalization`: `actor_obs_normalizer` / `critic_obs_normalizer` are an
    `EmpiricalNormalization` when the flag is on and `nn.Identity()` (no keys) when it is off; neither has a trainable parameter."""

    def __init__(self, obs_dim, critic_obs_dim, act_dim, actor_hidden=(512, 256, 128), critic_hidden=(512, 256, 128), init_noise_std=1.0,
                 actor_obs_normalization=False, critic_obs_normalization=False):
        super().__init__()
        self.actor = mlp([obs_dim, *actor_hidden, act_dim])
        self.critic = mlp([critic_obs_dim, *critic_hidden, 1])
        self.std = nn.Parameter(init_noise_std * torch.ones(act_dim))
        self.actor_obs_normalization, self.critic_obs_normalization = bool(actor_obs_normalization), bool(critic_obs_normalization)
        self.actor_obs_normalizer = EmpiricalNormalization(obs_dim) if actor_obs_normalization else nn.Identity()
        self.critic_obs_normalizer = EmpiricalNormalization(critic_obs_dim) if critic_obs_normalization else nn.Identity()

    def distribution(self, obs, normalized=False):
        """`normalized`: `obs` went through the actor's normaliser already"""
        mean = self.actor(obs if normalized else self.actor_obs_normalizer(obs))
        return mean, self.std.expand_as(mean)

    def evaluate(self, critic_obs):
        return self.critic(self.critic_obs_normalizer(critic_obs))

    def update_normalization(self, obs, critic_obs):
        """rsl_rl `ActorCritic.update_normalization`, what `process_env_step` calls with the NEW observations"""
        if self.actor_obs_normalization:
            self.actor_obs_normalizer.update(obs)
        if self.critic_obs_normalization:
            self.critic_obs_normalizer.update(critic_obs)


def gaussian_log_prob(actions, mean, std):
    """sum over the action dimensions of log N(a; mean, std^2) - torch.distributions.Normal(mean, std).log_prob(a).sum(-1)"""
    var = std * std
    return (-0.5 * (actions - mean) ** 2 / var - torch.log(std) - 0.9189385332046727).sum(-1)


def gaussian_entropy(std):
    return (0.5 + 0.9189385332046727 + torch.log(std)).sum(-1)


def gaussian_kl(mu_old, sigma_old, mu, sigma):
    """KL(old || new) of diagonal Gaussians, summed over the action dimensions (rsl_rl PPO.update's adaptive-schedule statistic)."""
    return (torch.log(sigma / sigma_old + 1e-5) + (sigma_old * sigma_old + (mu_old - mu) ** 2) / (2.0 * sigma * sigma) - 0.5).sum(-1)


def check_mirror_loss(who, symmetry, mirror_loss, data_augmentation):
    """(coefficient | None, data_augmentation) of a learner's `mirror_loss=` / `data_augmentation=` keywords, or a ValueError that says why"""
    data_augmentation = bool(data_augmentation)
    if mirror_loss is None:
        if symmetry is not None and not data_augmentation:
            raise ValueError(f"{who}: data_augmentation=False without mirror_loss leaves the symmetry tables with nothing to do "
                             "(pass mirror_loss=<coefficient>, or drop symmetry=)")
        return None, data_augmentation
    if isinstance(mirror_loss, bool) or not isinstance(mirror_loss, numbers.Real) or not math.isfinite(mirror_loss) or not mirror_loss > 0:
        raise ValueError(f"{who}: mirror_loss must be None (off) or a finite coefficient > 0, not {mirror_loss!r}")
    if symmetry is None:
        raise ValueError(f"{who}: mirror_loss needs symmetry= (the tables that say what the mirrored observation and action are)")
    if symmetry.n_sym < 2:
        raise ValueError(f"{who}: mirror_loss needs tables with n_sym >= 2 (the identity alone has no mirrored copy to compare with)")
    return float(mirror_loss), data_augmentation


class PPO:
    """`PPO.update()` of rsl_rl on a `robot_lab_amd.rollout.RolloutStorage` that `Collector.collect()` has filled
    (observations, privileged_observations, actions, values, returns, advantages, actions_log_prob, mu, sigma: [T, N, ...] views of
    the HIP storage; advantages already normalised over the batch by `rl_rollout_compute_returns`)."""

    def __init__(self, policy: ActorCritic, value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01,
                 num_learning_epochs=5, num_mini_batches=4, learning_rate=1.0e-3, schedule="adaptive", desired_kl=0.01, max_grad_norm=1.0,
                 group=None, symmetry=None, mirror_loss=None, data_augmentation=True, rnd=None):
        self.policy = policy
        # random network distillation (rsl_rl `rnd_cfg`): a robot_lab_amd.rnd.RandomNetworkDistillation whose predictor takes one step of a
        # separate Adam per mini-batch, on the mini-batch's rows (`update`); None: the code path of a learner built without the keyword
        self.rnd, self.rnd_optimizer = rnd, None
        if rnd is not None:
            from .rnd import RandomNetworkDistillation, make_optimizer

            if not isinstance(rnd, RandomNetworkDistillation):
                raise TypeError(f"PPO: rnd must be a robot_lab_amd.rnd.RandomNetworkDistillation (or None), not {type(rnd).__name__}")
            if symmetry is not None:
                raise NotImplementedError("PPO: rnd= with symmetry= is not implemented: whether the predictor trains on the mirrored copies is not decided here")
            self.rnd_optimizer = make_optimizer(rnd)
        # symmetry data augmentation (rsl_rl `use_data_augmentation=True`): a robot_lab_amd.symmetry.SymmetryTables, or None (the rule below
        # with one copy - the code path of a learner built without the keyword)
        if symmetry is not None:
            from .symmetry import SymmetryTables

            if not isinstance(symmetry, SymmetryTables):
                raise TypeError(f"PPO: symmetry must be a robot_lab_amd.symmetry.SymmetryTables (or None), not {type(symmetry).__name__}")
            lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
            symmetry.check_widths(lin(policy.actor)[0].in_features, lin(policy.critic)[0].in_features, policy.std.numel())
        self.symmetry = symmetry
        # rsl_rl's mirror loss (`use_mirror_loss`, `mirror_loss_coeff`) on the same tables: None (off) or the coefficient; `data_augmentation=False`
        # keeps the PPO terms on the stored rows (rsl_rl `use_data_augmentation=False`), see `update`
        self.mirror_loss, self.data_augmentation = check_mirror_loss("PPO", symmetry, mirror_loss, data_augmentation)
        self._sym_tensors = {}
        self.group = group  # robot_lab_amd.dist.LearnerGroup of a multi-GPU run (rsl_rl's gradient all-reduce); None = single learner
        self.value_loss_coef, self.use_clipped_value_loss, self.clip_param, self.entropy_coef = value_loss_coef, use_clipped_value_loss, clip_param, entropy_coef
        self.num_learning_epochs, self.num_mini_batches = num_learning_epochs, num_mini_batches
        self.learning_rate, self.schedule, self.desired_kl, self.max_grad_norm = learning_rate, schedule, desired_kl, max_grad_norm
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate)

    def _mirrored(self, which, x):
        """THE RULE of the augmentation, for one tensor of a mini-batch: [n, dim] -> [n_sym n, dim], copy s - S_s(x)[c] = sign[s][c] x[perm[s][c]],
        s = 0 the identity - in rows s n .. (s + 1) n.  A `None` table (the critic's observations) replicates the rows unchanged."""
        table = getattr(self.symmetry, which)
        if table is None:
            return x.repeat(self.symmetry.n_sym, 1)
        key = (which, x.device, x.dtype)
        if key not in self._sym_tensors:
            self._sym_tensors[key] = (torch.as_tensor(table[0].copy(), device=x.device, dtype=torch.long), torch.as_tensor(table[1].copy(), device=x.device, dtype=x.dtype))
        perm, sign = self._sym_tensors[key]
        return torch.cat([sign[s] * x[:, perm[s]] for s in range(perm.shape[0])], 0)

    def minibatch_loss(self, stats, mb_actions, mean, std, value, n, logp_old, adv, values, returns, mu_old, sigma_old, mirror=None):
        """The loss of one mini-batch from the networks' outputs on its rows (`mean`, `std`, `value`) and the stored quantities of the same rows
        (`mu_old` / `sigma_old`: of the first `n`, the stored copy): log-probability, entropy, the KL statistic and the adaptive learning rate it
        drives, the clipped surrogate, the (clipped) value loss.  The statistics are accumulated into `stats`.  One copy: the feed-forward update
        below and the recurrent one (robot_lab_amd/recurrent.py) differ only in how `mean` and `value` were computed."""
        logp = gaussian_log_prob(mb_actions, mean, std)
        entropy = gaussian_entropy(std)
        if self.schedule == "adaptive" and self.desired_kl is not None:
            with torch.inference_mode():
                kl = gaussian_kl(mu_old, sigma_old, mean[:n], std[:n]).mean()
                if self.group is not None:
                    kl = self.group.mean(kl)  # the same statistic on every rank -> the same learning rate on every rank
                if kl > 2.0 * self.desired_kl:
                    self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                elif 0.0 < kl < self.desired_kl / 2.0:
                    self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                for g in self.optimizer.param_groups:
                    g["lr"] = self.learning_rate
                stats["kl"] += float(kl)
        ratio = torch.exp(logp - logp_old)
        a = adv
        surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
        if self.use_clipped_value_loss:
            v_clipped = values + (value - values).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((value - returns) ** 2, (v_clipped - returns) ** 2).mean()
        else:
            value_loss = ((returns - value) ** 2).mean()
        loss = surrogate + self.value_loss_coef * value_loss - self.entropy_coef * entropy.mean()
        if mirror is not None:
            loss = loss + self.mirror_loss * mirror
            stats["mirror_loss"] += float(mirror.detach())
        stats["value_loss"] += float(value_loss.detach())
        stats["surrogate_loss"] += float(surrogate.detach())
        stats["entropy"] += float(entropy.detach().mean())
        return loss

    def optimizer_step(self, loss):
        """backward, the group's all-reduce, the clipped gradient norm, Adam, the floor of std"""
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.group is not None:
            self.group.reduce_gradients(self.policy)  # SUM / world, one flat all-reduce (rsl_rl `reduce_parameters`)
        nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
        self.optimizer.step()
        # a standard deviation pushed to (or through) zero would put NaN into the log-densities: the PARAMETER is floored, so that the
        # collector's sampling kernel, the stored sigma and this update all see the same distribution (rsl_rl 3.0.1 does not
        # clamp at all and fails with torch's Normal on a non-positive std; 1e-6 is far below any std training reaches)
        with torch.no_grad():
            self.policy.std.clamp_(min=1e-6)

    def update(self, storage, generator: torch.Generator | None = None) -> dict:
        """With `symmetry`: every mini-batch of n rows is evaluated on n_sym n rows - observations, critic observations and actions mirrored
        (`_mirrored`), old log-prob, advantage, return and value of a row repeated for each of its copies; both losses are means over the
        n_sym n rows (the entropy term does not change: the scalar std is the same for every row); the KL statistic that drives the adaptive
        learning rate stays the mean over the n stored rows (copy 0) against their stored mu / sigma.  Permutation draw, epochs x
        mini-batches, gradient clipping, Adam, the floor of std and the `group` all-reduce are those of the plain update.

        With `mirror_loss=c` (rsl_rl's `use_mirror_loss`, `mirror_loss_coeff`): mu_s = actor(S_s^obs(o)) for every copy s, the target
        tau_s = S_s^act(mu_0) DETACHED, L_mirror = mean over copies s >= 1, rows and action dimensions of (mu_s - tau_s)^2 (copy 0 is skipped, as
        rsl_rl's `mse_loss(mean_actions_batch[n:], actions_mean_symm_batch.detach()[n:])` does), and the loss gains c L_mirror; the result has one
        more key, `mirror_loss`: the mean over the mini-batches of L_mirror, before the coefficient.  `data_augmentation=True`: the PPO terms are
        the augmented ones above and the mu_s are the actor outputs the surrogate uses.  `data_augmentation=False`: surrogate, value loss, entropy
        and KL are those of a learner without symmetry - means over the n stored rows, the critic sees n rows - and the actor is additionally
        evaluated on copies 1 .. n_sym - 1 for L_mirror alone."""
        T, N = storage.num_transitions_per_env, storage.num_envs
        flat = lambda t: t.reshape(T * N, *t.shape[2:])  # noqa: E731
        obs, cobs, actions = flat(storage.observations), flat(storage.privileged_observations), flat(storage.actions)
        values, returns, adv = flat(storage.values).view(-1), flat(storage.returns).view(-1), flat(storage.advantages).view(-1)
        logp_old, mu_old, sigma_old = flat(storage.actions_log_prob).view(-1), flat(storage.mu), flat(storage.sigma)
        B = T * N
        mb = B // self.num_mini_batches
        # THE RULE with observation normalisation: actor(actor_obs_normalizer(obs)), critic(critic_obs_normalizer(critic_obs)) on the RAW stored rows.
        # A batch that says `obs_normalized` (Trainer's `NormalizedBatch`: both matrices already went through rl_obsnorm_apply, same bits as
        # the modules' forward) meets the networks directly.
        distribution, critic = self.policy.distribution, self.policy.evaluate
        if getattr(storage, "obs_normalized", False):
            distribution, critic = functools.partial(distribution, normalized=True), self.policy.critic
        stats = dict(value_loss=0.0, surrogate_loss=0.0, entropy=0.0, kl=0.0)
        if self.mirror_loss is not None:
            stats["mirror_loss"] = 0.0
        n_updates = 0
        if self.rnd is not None:  # the stored o_t of the RND group; the statistic is the mean over the mini-batches of the predictor's loss
            from .rnd import storage_state, update_minibatch

            rnd_state = storage_state(storage, self.rnd.group)
            stats["rnd_loss"] = 0.0
        # rsl_rl's `mini_batch_generator` draws ONE permutation per update and walks it once per epoch
        perm = torch.randperm(B, device=obs.device, generator=generator)
        for _ in range(self.num_learning_epochs):
            for i in range(self.num_mini_batches):
                idx = perm[i * mb:(i + 1) * mb]
                if self.symmetry is None:
                    mb_obs, mb_cobs, mb_actions, rep = obs[idx], cobs[idx], actions[idx], idx
                elif not self.data_augmentation:  # the actor on every copy (the mirror loss), everything else on the stored rows
                    mb_obs, mb_cobs, mb_actions, rep = self._mirrored("obs", obs[idx]), cobs[idx], actions[idx], idx
                else:
                    mb_obs, mb_cobs, mb_actions = self._mirrored("obs", obs[idx]), self._mirrored("critic", cobs[idx]), self._mirrored("act", actions[idx])
                    rep = idx.repeat(self.symmetry.n_sym)  # the stored row of every one of the n_sym n rows
                n = idx.numel()
                mean, std = distribution(mb_obs)
                if self.mirror_loss is not None:
                    mirror = ((mean[n:] - self._mirrored("act", mean[:n].detach())[n:]) ** 2).mean()
                    if not self.data_augmentation:
                        mean, std = mean[:n], std[:n]
                value = critic(mb_cobs).view(-1)
                loss = self.minibatch_loss(stats, mb_actions, mean, std, value, n, logp_old[rep], adv[rep], values[rep], returns[rep], mu_old[idx], sigma_old[idx],
                                           mirror if self.mirror_loss is not None else None)
                self.optimizer_step(loss)
                if self.rnd is not None:  # the same rows, a separate Adam on the predictor alone: no clipping, no adaptive learning rate
                    stats["rnd_loss"] += update_minibatch(self.rnd, self.rnd_optimizer, rnd_state[idx])
                n_updates += 1
        out = {k: v / max(n_updates, 1) for k, v in stats.items()}
        out["learning_rate"] = self.learning_rate
        return out


def mirror_repr(alg):
    """what a `repr` that prints the symmetry adds for the mirror loss"""
    if alg.mirror_loss is None:
        return ""
    return f", mirror_loss={alg.mirror_loss:g}" + ("" if alg.data_augmentation else ", data_augmentation=False")


class NormalizedBatch:
    """A filled `RolloutStorage` as the learners read it, with `observations` / `privileged_observations` replaced by matrices that
    `normalize()` fills with `rl_obsnorm_apply` over all T N stored rows (a group without normaliser keeps the storage's own tensor);
    every other attribute is the storage's.  `obs_normalized` tells `PPO.update` that the modules' forward has been applied already."""
    obs_normalized = True

    def __init__(self, storage, normalizers):
        self._storage, self._normalizers = storage, normalizers
        raw = (storage.observations, storage.privileged_observations)
        self._raw = raw
        self.observations, self.privileged_observations = (r if h is None else torch.empty_like(r) for r, h in zip(raw, normalizers))

    def __getattr__(self, name):
        return getattr(self._storage, name)

    def normalize(self):
        for h, r, out in zip(self._normalizers, self._raw, (self.observations, self.privileged_observations)):
            if h is not None:
                h.apply(r.view(-1, r.shape[-1]), out=out.view(-1, out.shape[-1]))


MAX_INPUT_WIDTH = 512  # = RL_MLP_MAX_WIDTH (include/rl_policy.h) = RL_PPO_MAX_WIDTH (include/rl_ppo.h): widest layer, the input included


RECURRENT_LEARNERS = ("torch", "hip")


def check_recurrent_trainer(rnn_type, rnn_hidden_dim, rnn_num_layers, critic_group, learner, symmetry, group, normalization, ppo_kw, recurrent_learner="torch"):
    """What `Trainer(rnn_type=...)` does not combine with is refused with a reason, never ignored (no device needed)."""
    from .recurrent import check_rnn_cfg

    check_rnn_cfg("Trainer", rnn_type, rnn_hidden_dim, rnn_num_layers)
    if critic_group not in ("critic", "policy"):
        raise ValueError(f"Trainer: critic_group must be \"critic\" or \"policy\", not {critic_group!r}")
    if recurrent_learner not in RECURRENT_LEARNERS:
        raise ValueError(f"Trainer: recurrent_learner must be \"torch\" or \"hip\", not {recurrent_learner!r}")
    if learner == "hip":
        raise NotImplementedError("Trainer: learner=\"hip\" with a recurrent policy is not implemented: learner= names the feed-forward learners, and "
                                  "back-propagation through time in the HIP learner has a switch of its own - pass recurrent_learner=\"hip\" "
                                  "(robot_lab_amd/recurrent_hip.py) and leave learner= at \"torch\"")
    if learner != "torch":
        raise ValueError(f"learner must be \"torch\" or \"hip\", not {learner!r}")
    if symmetry is not None or ppo_kw.get("mirror_loss") is not None:
        raise NotImplementedError("Trainer: symmetry= / mirror_loss= with a recurrent policy is not implemented: mirroring a trajectory through the memory (whose "
                                  "saved state has no mirror table) is not defined here; drop symmetry= or rnn_type=")
    if normalization:
        raise NotImplementedError("Trainer: the observation-normalisation flags with a recurrent policy are not implemented: the statistics' update would sit "
                                  "between the cell launch and its state record inside the captured loop; drop the *_obs_normalization flags or rnn_type=")
    if group is not None and getattr(group, "world_size", 1) > 1:
        raise NotImplementedError(f"Trainer: a recurrent policy with a group of {group.world_size} ranks is not implemented: the recurrent update walks "
                                  "contiguous blocks of envs in order and the ranks' gradient exchange per block is not decided here; run one rank")


class Trainer:
    """collect (HIP, one graph launch) -> update -> push parameters, repeated: `OnPolicyRunner.learn` in miniature.
    `learner="torch"` (default): `PPO` above, autograd; `learner="hip"`: `ppo_hip.HipPPO`, the same rule as HIP kernels (with a `group`: its split update
    around the group's all-reduce), pushed into the inference kernels device to device; `state_dict()` is rsl_rl's layout with either.
    `symmetry`: symmetry data augmentation inside the update of either learner - a `symmetry.SymmetryTables`, or the mirrors of this
    env's robot ("lr", "fb", "lr,fb" or a tuple of them), resolved with `symmetry.tables_for_env(env)`.
    `mirror_loss=c`, `data_augmentation=False` (with `symmetry`; forwarded to the learner): rsl_rl's mirror loss on the same tables, with
    or without the augmentation - the rule is `PPO.update`'s.
    `actor_obs_normalization`, `critic_obs_normalization`: rsl_rl's empirical normalisation of the group (`EmpiricalNormalization` is the
    rule, csrc/rl_obsnorm.hip runs it): statistics updated inside the captured collection loop with the NEW observations of every step,
    applied in front of both networks there, and once per update over the stored RAW rows with the statistics as the collection left
    them.  `state_dict()` gains rsl_rl's `actor_obs_normalizer.*` / `critic_obs_normalizer.*` keys.  Refused with a `group` of more than
    one rank, and - unless `normalize_in_learner` - with `symmetry`.
    `normalize_in_learner=True` (with a normalisation flag): the update reads the RAW storage and the learner normalises - the torch learner
    through the modules' forward, the HIP learner in its first layer's operand fetch (`HipPPO(obs_normalizers=...)`), both behind the mirror, as
    rsl_rl does: the mirrored raw row is normalised.  No normalised copy of the batch is allocated.  This is what `symmetry` / `mirror_loss`
    need together with normalised observations; the default stays the scratch matrices of `NormalizedBatch`.
    `rnn_type="lstm"`, `rnn_hidden_dim`, `rnn_num_layers=1`, `critic_group="critic" | "policy"`: a recurrent policy (rsl_rl `ActorCriticRecurrent`; the rule
    is robot_lab_amd/recurrent.py) - `actor_hidden` / `critic_hidden` are then the MLP heads behind the two memories.  The cells run as HIP kernels in
    the captured collection loop, the update is `recurrent.RecurrentPPO` (torch) or, with `recurrent_learner="hip"`, `recurrent_hip.HipRecurrentPPO`:
    back-propagation through time as HIP kernels (include/rl_bptt.h), pushed into cells and heads device to device.  Refused with `learner="hip"`
    (that keyword names the feed-forward learners), "gru", several layers, `symmetry`, the normalisation flags and a `group` of more than one rank;
    `recurrent_learner` without `rnn_type` is refused too.
    `rnd=dict(weight, weight_schedule=None, reward_normalization=False, state_normalization=False, learning_rate=1e-3, num_outputs=1, predictor_hidden_dims,
    target_hidden_dims, group="policy")`: random network distillation (rsl_rl's `rnd_cfg`; the rule is robot_lab_amd/rnd.py) - the intrinsic reward is added to
    the stored rewards inside the captured collection loop (csrc/rl_rnd.hip), the predictor takes one step of a separate Adam per mini-batch of the update of
    either learner (`learner="hip"`: include/rl_rnd_learner.h).  `iterate()` gains `rnd_loss`, `mean_intrinsic_reward`, `mean_extrinsic_reward`, `rnd_weight`.
    Refused with `rnn_type`, `symmetry` / `mirror_loss`, the normalisation flags, a `group` of more than one rank, hidden dims of -1, more than one state group."""

    def __init__(self, env, num_steps_per_env=24, gamma=0.99, lam=0.95, seed=1, use_graph=True, actor_hidden=(512, 256, 128),
                 critic_hidden=(512, 256, 128), init_noise_std=1.0, clip_actions=None, group=None, learner="torch", symmetry=None,
                 actor_obs_normalization=False, critic_obs_normalization=False, normalize_in_learner=False, rnn_type=None, rnn_hidden_dim=256,
                 rnn_num_layers=1, critic_group="critic", recurrent_learner="torch", rnd=None, **ppo_kw):
        from .collect import Collector
        from .policy import MlpPolicy
        from .rollout import RolloutStorage

        self.recurrent = None
        self.rnd = self.rnd_device = self.rnd_learner = None
        rnd_kw = None
        if rnd is not None:  # refused before the env is touched: what random network distillation does not combine with
            from .rnd import check_rnd_trainer

            rnd_kw = check_rnd_trainer(rnd, rnn_type, symmetry, ppo_kw, actor_obs_normalization or critic_obs_normalization or normalize_in_learner, group)
            if learner not in ("torch", "hip"):
                raise ValueError(f"learner must be \"torch\" or \"hip\", not {learner!r}")
        if rnn_type is not None:  # refused before the env is touched: what a recurrent policy does not combine with
            check_recurrent_trainer(rnn_type, rnn_hidden_dim, rnn_num_layers, critic_group, learner, symmetry, group,
                                    actor_obs_normalization or critic_obs_normalization or normalize_in_learner, ppo_kw, recurrent_learner)
        elif recurrent_learner != "torch":
            if recurrent_learner not in RECURRENT_LEARNERS:
                raise ValueError(f"Trainer: recurrent_learner must be \"torch\" or \"hip\", not {recurrent_learner!r}")
            raise NotImplementedError(f"Trainer: recurrent_learner={recurrent_learner!r} is read by a recurrent policy only (rnn_type=\"lstm\"); the learner of a "
                                      "feed-forward policy is learner=")
        elif critic_group != "critic":
            raise NotImplementedError("Trainer: critic_group is read by a recurrent policy only (rnn_type=\"lstm\"); the feed-forward critic reads the critic group")
        obs, _ = env.reset()
        od, cd, A = obs["policy"].shape[1], obs[critic_group].shape[1], env.num_actions
        if rnd_kw is not None:
            from .rnd import check_state_width

            check_state_width(rnd_kw["group"], obs[rnd_kw["group"]].shape[1])
        for name, width in (("policy", od), ("critic", cd)):  # before anything is built: the kernels would fail deep inside otherwise
            if width > MAX_INPUT_WIDTH:
                hist = (getattr(env, "obs_history", None) or {}).get(name)
                raise ValueError(f"Trainer: the {name} observation row is {width} columns wide" + (f" (observation history {hist})" if hist else "") +
                                 f", the fused inference kernels and the HIP learner take at most {MAX_INPUT_WIDTH} input columns: shorten the "
                                 f"{name} group's history_length or drop terms from it")
        normalized = tuple(name for name, on in (("policy", actor_obs_normalization), ("critic", critic_obs_normalization)) if on)
        normalize_in_learner = bool(normalize_in_learner)
        if normalize_in_learner and not normalized:
            raise ValueError("Trainer: normalize_in_learner=True without actor_obs_normalization / critic_obs_normalization: there is nothing to normalise")
        if normalized and symmetry is not None and not normalize_in_learner:
            raise NotImplementedError("Trainer: symmetry= together with observation normalisation needs normalize_in_learner=True: rsl_rl normalises the "
                                      "MIRRORED raw row, which is not the mirror of the normalised row unless the statistics are symmetric, and by default "
                                      "the learners read a batch that was normalised before their first layer's operand fetch mirrors it "
                                      "(pass normalize_in_learner=True, or drop symmetry= or the *_obs_normalization flags)")
        if normalized and group is not None and getattr(group, "world_size", 1) > 1:
            raise NotImplementedError(f"Trainer: observation normalisation with a group of {group.world_size} ranks is not implemented: whether the ranks "
                                      "keep their own statistics or reduce them is not decided here (run one rank, or drop the *_obs_normalization flags)")
        torch.manual_seed(seed)
        self.env, self.device = env, obs["policy"].device
        if rnn_type is not None:
            self._init_recurrent(env, od, cd, A, num_steps_per_env, gamma, lam, seed, use_graph, actor_hidden, critic_hidden, init_noise_std, clip_actions,
                                 rnn_type, rnn_hidden_dim, rnn_num_layers, critic_group, ppo_kw, recurrent_learner)
            return
        if normalized:
            self.policy = ActorCritic(od, cd, A, tuple(actor_hidden), tuple(critic_hidden), init_noise_std, bool(actor_obs_normalization),
                                      bool(critic_obs_normalization)).to(self.device)
        else:
            self.policy = ActorCritic(od, cd, A, tuple(actor_hidden), tuple(critic_hidden), init_noise_std).to(self.device)
        self.normalized, self.normalize_in_learner = normalized, normalize_in_learner
        if learner not in ("torch", "hip"):
            raise ValueError(f"learner must be \"torch\" or \"hip\", not {learner!r}")
        self.learner = learner
        for refused in ("use_mirror_loss", "mirror_loss_coeff"):
            if refused in ppo_kw:
                raise NotImplementedError(f"Trainer: {refused} is rsl_rl's spelling and is not taken here: the mirror loss is "
                                          "Trainer(..., symmetry=..., mirror_loss=<coefficient>, data_augmentation=True | False)")
        if symmetry is not None:  # None | SymmetryTables | a mirror spec for this env's robot: "lr", "fb", "lr,fb", ("lr", "fb")
            from .symmetry import SymmetryTables, tables_for_env

            if not isinstance(symmetry, SymmetryTables):
                symmetry = tables_for_env(env, symmetry)
            ppo_kw["symmetry"] = symmetry
        self.symmetry = symmetry
        self.normalizers = None
        if normalized:  # the device half of the policy's EmpiricalNormalization modules
            from .obsnorm import ObsNormalizer

            mods = (self.policy.actor_obs_normalizer, self.policy.critic_obs_normalizer)
            self.normalizers = tuple(ObsNormalizer(m._mean.shape[1], m.eps, max_rows=env.num_envs, device=str(self.device)) if isinstance(m, EmpiricalNormalization)
                                     else None for m in mods)
            if normalize_in_learner and learner == "hip":
                ppo_kw["obs_normalizers"] = self.normalizers  # (the torch learner runs the modules' forward on the raw batch)
        if rnd_kw is not None:
            # built AFTER the policy (whose initial parameters are therefore those of a Trainer without rnd=), before the learner that trains it
            from .rnd import RandomNetworkDistillation
            from .rnd_hip import HipRND, RndDevice

            g = rnd_kw.pop("group")
            self.rnd = RandomNetworkDistillation(od if g == "policy" else cd, group=g, **rnd_kw).to(self.device)
            self.rnd_device = RndDevice(self.rnd, env.num_envs, num_steps_per_env, device=str(self.device))
            if learner == "hip":
                self.rnd_learner = HipRND(self.rnd, ppo_kw.get("num_learning_epochs", 5), ppo_kw.get("num_mini_batches", 4),
                                          max(1, num_steps_per_env * env.num_envs // ppo_kw.get("num_mini_batches", 4)), state_normalizer=self.rnd_device.state_norm)
            ppo_kw["rnd"] = self.rnd_learner if learner == "hip" else self.rnd
        if learner == "hip":
            from .ppo_hip import HipPPO

            self.alg = HipPPO(self.policy, group=group, max_rows_per_minibatch=max(1, num_steps_per_env * env.num_envs // ppo_kw.get("num_mini_batches", 4)), **ppo_kw)
        else:
            self.alg = PPO(self.policy, group=group, **ppo_kw)
        if group is not None:
            group.broadcast_parameters(self.policy)  # before the inference images are built from them
            if learner == "hip":
                self.alg.load_from(self.policy)  # ... and into the HIP learner's master parameters, which were copied before the broadcast
        lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        self.actor = MlpPolicy([host(x.weight) for x in lin(self.policy.actor)], [host(x.bias) for x in lin(self.policy.actor)], "elu", device=str(self.device))
        self.critic = MlpPolicy([host(x.weight) for x in lin(self.policy.critic)], [host(x.bias) for x in lin(self.policy.critic)], "elu", device=str(self.device))
        self.storage = RolloutStorage(env.num_envs, num_steps_per_env, od, cd, A, seed=seed, device=str(self.device))
        self.std = self.policy.std.detach().clone()  # the tensor the sampling kernel reads: refreshed in place after every update
        self._batch = self.storage
        if normalized:
            if not normalize_in_learner:  # the update's normalised [T N, dim] matrices
                self._batch = NormalizedBatch(self.storage, self.normalizers)
            self.collector = Collector(env, self.actor, self.critic, self.storage, self.std, gamma=gamma, lam=lam, use_graph=use_graph, clip_actions=clip_actions,
                                       normalizers=self.normalizers)
        elif self.rnd_device is not None:
            self.collector = Collector(env, self.actor, self.critic, self.storage, self.std, gamma=gamma, lam=lam, use_graph=use_graph, clip_actions=clip_actions,
                                       rnd=self.rnd_device)
        else:
            self.collector = Collector(env, self.actor, self.critic, self.storage, self.std, gamma=gamma, lam=lam, use_graph=use_graph, clip_actions=clip_actions)
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        self.iteration = 0

    def _init_recurrent(self, env, od, cd, A, num_steps_per_env, gamma, lam, seed, use_graph, actor_hidden, critic_hidden, init_noise_std, clip_actions,
                        rnn_type, rnn_hidden_dim, rnn_num_layers, critic_group, ppo_kw, recurrent_learner="torch"):
        """`rnn_type="lstm"`: `recurrent.ActorCriticRecurrent` under `recurrent.RecurrentPPO` (torch) or - `recurrent_learner="hip"` -
        `recurrent_hip.HipRecurrentPPO` (back-propagation through time as HIP kernels), the two cells (csrc/rl_lstm.hip) and the MLP heads of input
        width H in the recurrent `Collector`; all of them are pushed after every update."""
        from .collect import Collector
        from .lstm import LstmCell, RecurrentState
        from .policy import MlpPolicy
        from .recurrent import ActorCriticRecurrent, RecurrentBatch, RecurrentPPO
        from .rollout import RolloutStorage

        self.policy = ActorCriticRecurrent(od, cd, A, tuple(actor_hidden), tuple(critic_hidden), init_noise_std, rnn_type, rnn_hidden_dim, rnn_num_layers).to(self.device)
        self.normalized, self.normalize_in_learner, self.normalizers, self.symmetry, self.learner = (), False, None, None, "torch"
        self.recurrent_learner = recurrent_learner
        if recurrent_learner == "hip":
            from .recurrent_hip import HipRecurrentPPO

            self.alg = HipRecurrentPPO(self.policy, num_steps=num_steps_per_env, num_envs=env.num_envs, **ppo_kw)
        else:
            self.alg = RecurrentPPO(self.policy, **ppo_kw)
        lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        dev = str(self.device)
        self.actor = MlpPolicy([host(x.weight) for x in lin(self.policy.actor)], [host(x.bias) for x in lin(self.policy.actor)], "elu", device=dev)
        self.critic = MlpPolicy([host(x.weight) for x in lin(self.policy.critic)], [host(x.bias) for x in lin(self.policy.critic)], "elu", device=dev)
        self.recurrent = RecurrentState(LstmCell.from_module(self.policy.memory_a.rnn, device=dev), LstmCell.from_module(self.policy.memory_c.rnn, device=dev),
                                        env.num_envs, num_steps_per_env)
        self.recurrent.critic_group = critic_group
        self.storage = RolloutStorage(env.num_envs, num_steps_per_env, od, cd, A, seed=seed, device=dev)
        self.std = self.policy.std.detach().clone()
        rec = self.recurrent
        self._batch = RecurrentBatch(self.storage, (rec.h_a[0], rec.c_a[0]), (rec.h_c[0], rec.c_c[0]))
        self.collector = Collector(env, self.actor, self.critic, self.storage, self.std, gamma=gamma, lam=lam, use_graph=use_graph, clip_actions=clip_actions,
                                   recurrent=rec)
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        self.iteration = 0

    def __repr__(self):
        sym = f", symmetry={self.symmetry!r}{mirror_repr(self.alg)}" if self.symmetry is not None else ""
        sym += f", recurrent=lstm({self.policy.rnn_hidden_dim}), recurrent_learner={self.recurrent_learner!r}" if self.recurrent is not None else ""
        sym += f", obs_normalization={list(self.normalized)}" if self.normalized else ""
        sym += ", normalize_in_learner=True" if self.normalize_in_learner else ""
        sym += f", rnd={self.rnd.group!r}" if self.rnd is not None else ""
        return f"Trainer(learner={self.learner!r}, alg={type(self.alg).__name__}, num_envs={self.env.num_envs}, iteration={self.iteration}{sym})"

    def _modules(self):
        if self.recurrent is not None:
            return ()
        return (self.policy.actor_obs_normalizer, self.policy.critic_obs_normalizer)

    def sync_normalizers(self):
        """the normalisers' device state into the policy's `EmpiricalNormalization` buffers (stream-ordered, no wait)"""
        for h, m in zip(self.normalizers or (), self._modules()):
            if h is not None:
                h.store_module(m)

    def state_dict(self):
        """rsl_rl's `ActorCritic.state_dict()` layout; the HIP learner's master parameters and the normalisers' device state are copied
        back into the module first."""
        if self.learner == "hip":
            self.alg.store_into(self.policy)
        if self.recurrent is not None and self.recurrent_learner == "hip":
            self.alg.sync_policy()
        self.sync_normalizers()
        return self.policy.state_dict()

    def push_parameters(self):
        """the module's parameters into the inference kernels and - after a `load_state_dict` - its normaliser buffers into the handles"""
        if self.rnd_device is not None:  # the target and RND's normalisers' buffers; the predictor too unless the HIP learner holds it (pushed below)
            self.rnd_device.load_module(predictor=self.rnd_learner is None)
        self._push_weights()
        for h, m in zip(self.normalizers or (), self._modules()):
            if h is not None:
                h.load_module(m)

    def _push_weights(self):
        if self.rnd_device is not None:  # the predictor the next collection's intrinsic reward runs (the same stream ordering as below)
            if self.rnd_learner is not None:
                self.rnd_learner.push(self.rnd_device.predictor)
            else:
                self.rnd_device.predictor.load_linear_layers(self.rnd.predictor)
        if self.learner == "hip":
            # Device to device on the CURRENT stream, with no device-wide wait (unlike rl_mlp_set_weights below).  Ordering relied on: the update
            # ran on this stream, so the push follows it; the next collection - eager or the captured graph - is launched on this same stream, so
            # it follows the push; with Collector(overlap=True) the critic's side stream waits for this stream at the head of every step
            # (collect.py: side.wait_stream(main)), in the capture too.  A collector launched from ANOTHER stream would have to wait for this one.
            self.alg.push(self.actor, self.critic, self.std)
            return
        if self.recurrent is not None and self.recurrent_learner == "hip":  # the same ordering: cells, heads and std read the flat buffer in place
            self.alg.push(self.recurrent.cell_a, self.recurrent.cell_c, self.actor, self.critic, self.std)
            return
        self.actor.load_linear_layers(self.policy.actor)
        self.critic.load_linear_layers(self.policy.critic)
        self.std.copy_(self.policy.std.detach().clamp_min(1e-6))
        if self.recurrent is not None:  # device to device on this stream, which the next collection follows (rl_lstm_set_weights_device)
            self.recurrent.cell_a.load_module(self.policy.memory_a.rnn)
            self.recurrent.cell_c.load_module(self.policy.memory_c.rnn)

    def update_batch(self):
        """the filled storage as the learner reads it: the storage itself (no normalisation, or `normalize_in_learner`: the learner normalises the
        raw rows), or - with observation normalisation - a `NormalizedBatch` whose two observation matrices hold the stored raw rows through the
        statistics as the collection left them (one `apply` per group)"""
        if self.normalized:
            if not self.normalize_in_learner:
                self._batch.normalize()
            # `alg.policy`'s buffers stay current: the torch rule (with `normalize_in_learner` its forward over the raw batch), exporters and
            # checkpoints read them; the HIP learner reads the handles' own vectors
            self.sync_normalizers()
        if self.rnd_device is not None:  # the state statistics as the collection left them: what the torch rule's forward reads
            self.rnd_device.sync_module()
        return self._batch

    # -- random network distillation: rsl_rl's checkpoint entries `rnd_state_dict` / `rnd_optimizer_state_dict` ------------------------------
    def rnd_state_dict(self):
        """`RandomNetworkDistillation.state_dict()` (predictor.*, target.*, state_normalizer.*, reward_normalizer.*) with the HIP learner's master
        parameters and the normalisers' device state copied back first"""
        if self.rnd_learner is not None:
            self.rnd_learner.store_into(self.rnd)
        self.rnd_device.sync_module()
        return self.rnd.state_dict()

    def rnd_optimizer_state_dict(self):
        """the layout of `torch.optim.Adam(predictor.parameters()).state_dict()` with either learner"""
        return self.rnd_learner.optimizer_state_dict() if self.rnd_learner is not None else self.alg.rnd_optimizer.state_dict()

    def load_rnd_state(self, state_dict, optimizer_state_dict=None):
        """a checkpoint's RND entries, written under either learner, into the module, the device images and the learner"""
        self.rnd.load_state_dict(state_dict)
        self.rnd_device.load_module()
        if self.rnd_learner is not None:
            self.rnd_learner.load_from(self.rnd)
        if optimizer_state_dict:
            if self.rnd_learner is not None:
                self.rnd_learner.load_optimizer_state_dict(optimizer_state_dict)
            else:
                self.alg.rnd_optimizer.load_state_dict(optimizer_state_dict)

    def iterate(self) -> dict:
        self.collector.collect()
        st = self.storage
        out = dict(mean_reward=float(st.rewards.mean()), done_rate=float(st.dones.float().mean()))
        if self.rnd_device is not None:  # the fixed-order sums the reward kernels left (csrc/rl_rnd.hip); mean_reward above is their total
            intrinsic, total = self.rnd_device.reward.sums()
            count = st.num_transitions_per_env * st.num_envs
            out.update(mean_intrinsic_reward=intrinsic / count, mean_extrinsic_reward=(total - intrinsic) / count, rnd_weight=self.rnd_device.last_weight)
        out.update(self.alg.update(self.update_batch(), self.gen))
        self._push_weights()
        hip = self.learner == "hip" or (self.recurrent is not None and self.recurrent_learner == "hip")
        out["action_std"] = float((self.std if hip else self.policy.std.detach()).mean())
        self.iteration += 1
        return out
