"""Random network distillation (RND): rsl_rl's intrinsic curiosity reward, THE RULE in plain torch (CPU or GPU, fp32 or fp64).

[UPSTREAM] restated from rsl_rl 3.0.1 (`modules/rnd.py` `RandomNetworkDistillation`, `algorithms/ppo.py` `process_env_step` / `update`); rsl-rl-lib is
not in this tree and the rule below is not pinned to it.  The device half is csrc/rl_rnd.hip (the reward, inside the captured collection loop:
include/rl_rnd.h, robot_lab_amd/rnd_hip.py `RndDevice`) and csrc/learner/rl_rnd.inl (the predictor's update: include/rl_rnd_learner.h, `HipRND`);
both are checked against this file.

    rnd = RandomNetworkDistillation(state_dim, num_outputs=K, predictor_hidden_dims=..., target_hidden_dims=..., weight=w, ...)

Two ELU MLPs map the RND state - ONE observation group of the env - to K columns: a fixed random `target` and a `predictor` trained to match
it.  Where the predictor has not yet seen a state it is wrong, and the size of its error is the bonus.

Per collection step, after env.step, on the NEW observations o_{t+1} (post-reset rows for envs that were done) - `collect_step`:
    1. state normalisation on: update it with o_{t+1}; s = normalise(o_{t+1})          (`ppo.EmpiricalNormalization`, unchanged)
    2. r = || target(s) - predictor(s) ||_2 per row
    3. reward normalisation on: avg <- avg gamma_r + r per env (avg starts at 0), `EmpiricalNormalization(1).update(avg)` over the N values
       of the step, r <- r / std if std > 0 else r - the std AFTER this step's update, no eps, no mean
    4. r <- r weight_t, the weight following its schedule on the count of calls (this one included)
    5. rewards[t] += r
Step 5 is the one deliberate deviation: the env kernel has already added the time-out bootstrap gamma V_t to the slot, so the sum is
(r_ext + gamma V to) + r_int where rsl_rl forms (r_ext + r_int) + gamma V to - an fp32 rounding difference only.  The rule here uses the
device's order.

Per mini-batch of the PPO update, on the same rows `idx` of the same permutation - `update_minibatch`:
    under no grad s = normalise(state[idx]) with the statistics as the collection left them;
    L = mean over the n K entries of (predictor(s) - target(s).detach())^2; one step of a SEPARATE Adam (lr = learning_rate, default 1e-3,
    betas 0.9 / 0.999, eps 1e-8) on the predictor only: no gradient clipping, untouched by the adaptive KL schedule.
The PPO step of that mini-batch is unchanged; `PPO.update(..., )` with `rnd=` gains the key `rnd_loss`, the mean over the mini-batches."""
from __future__ import annotations

import math
import numbers

import torch
from torch import nn

from .ppo import EmpiricalNormalization, mlp

MAX_WIDTH, MAX_LAYERS = 512, 8  # what the fused inference kernels and the HIP learner take (include/rl_policy.h, include/rl_rnd_learner.h)
SCHEDULES = ("constant", "step", "linear")
RND_KEYS = ("weight", "weight_schedule", "reward_normalization", "state_normalization", "learning_rate", "num_outputs", "predictor_hidden_dims",
            "target_hidden_dims", "group")


def read_schedule(weight_schedule):
    """(mode, params) of a `weight_schedule`: None or "constant" (constant weight), or a dict / cfg object with `mode` = "constant" | "step"
    (`final_step`, `final_value`) | "linear" (`initial_step`, `final_step`, `final_value`) - IsaacLab's `RslRlRndCfg.*WeightScheduleCfg` fields."""
    if weight_schedule is None or weight_schedule == "constant":
        return "constant", {}
    get = weight_schedule.get if isinstance(weight_schedule, dict) else lambda k, d=None: getattr(weight_schedule, k, d)  # noqa: E731
    mode = get("mode") if not isinstance(weight_schedule, str) else weight_schedule
    if mode not in SCHEDULES:
        raise ValueError(f"rnd: weight_schedule mode {mode!r} is not one of {SCHEDULES}")
    if mode == "constant":
        return mode, {}
    if isinstance(weight_schedule, str):
        raise ValueError(f"rnd: weight_schedule={weight_schedule!r} needs its parameters: pass dict(mode={weight_schedule!r}, final_step=..., final_value=...)")
    names = ("final_step", "final_value") if mode == "step" else ("initial_step", "final_step", "final_value")
    params = {}
    for k in names:
        v = get(k)
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not math.isfinite(v):
            raise ValueError(f"rnd: weight_schedule mode {mode!r} needs a finite number {k}, got {v!r}")
        params[k] = v
    if mode == "linear" and not params["final_step"] > params["initial_step"]:
        raise ValueError(f"rnd: the linear weight_schedule needs final_step > initial_step, got {params['initial_step']} .. {params['final_step']}")
    return mode, params


def schedule_weight(initial_weight, mode, params, count):
    """the weight of the call that brings the count of calls to `count` (one call per env step), a Python float"""
    if mode == "constant":
        return float(initial_weight)
    if mode == "step":
        return float(initial_weight) if count < params["final_step"] else float(params["final_value"])
    lo, hi = params["initial_step"], params["final_step"]
    if count <= lo:
        return float(initial_weight)
    if count >= hi:
        return float(params["final_value"])
    return float(initial_weight + (params["final_value"] - initial_weight) * (count - lo) / (hi - lo))


class DiscountedRewardNormalization(nn.Module):
    """rsl_rl's `EmpiricalDiscountedVariationNormalization`: the intrinsic reward divided by the running std of its per-env discounted average.
    `state_dict()` keys: `emp_norm._mean`, `._var`, `._std`, `.count`; the per-env average `avg` is run state and no buffer, as upstream."""

    def __init__(self, gamma=0.99):
        super().__init__()
        self.gamma = float(gamma)
        self.emp_norm = EmpiricalNormalization(1)
        self.avg = None  # [N], 0 before the first step

    @torch.no_grad()
    def forward(self, r):
        if self.training:
            self.avg = r.clone() if self.avg is None else self.avg * self.gamma + r  # (0 gamma + r = r)
            self.emp_norm.update(self.avg.view(-1, 1))
        std = self.emp_norm._std.view(())
        return r / std if bool(std > 0) else r


class RandomNetworkDistillation(nn.Module):
    """`state_dict()` keys: `predictor.*`, `target.*`, `state_normalizer.*`, `reward_normalizer.*` (rsl_rl's).  The target is never trained."""

    def __init__(self, state_dim, num_outputs=1, predictor_hidden_dims=(256, 256), target_hidden_dims=(256, 256), weight=0.0, weight_schedule=None,
                 state_normalization=False, reward_normalization=False, reward_gamma=0.99, learning_rate=1e-3, group="policy"):
        super().__init__()
        self.state_dim, self.num_outputs, self.group = int(state_dim), int(num_outputs), group
        self.predictor = mlp([self.state_dim, *predictor_hidden_dims, self.num_outputs])
        self.target = mlp([self.state_dim, *target_hidden_dims, self.num_outputs])
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.state_normalization, self.reward_normalization = bool(state_normalization), bool(reward_normalization)
        self.state_normalizer = EmpiricalNormalization(self.state_dim) if state_normalization else nn.Identity()
        self.reward_normalizer = DiscountedRewardNormalization(reward_gamma) if reward_normalization else nn.Identity()
        self.initial_weight, self.learning_rate = float(weight), float(learning_rate)
        self.schedule = read_schedule(weight_schedule)
        self.update_counter = 0  # calls of `intrinsic_reward`: one per env step
        self.weight = self.initial_weight

    def weight_at(self, count):
        return schedule_weight(self.initial_weight, *self.schedule, count)

    @torch.no_grad()
    def raw_reward(self, new_state):
        """steps 1 and 2: (r [N], the normalised rows)"""
        if self.state_normalization:
            self.state_normalizer.update(new_state)
        s = self.state_normalizer(new_state)
        return torch.linalg.vector_norm(self.target(s) - self.predictor(s), dim=1), s

    @torch.no_grad()
    def intrinsic_reward(self, new_state):
        """steps 1 - 4 on the new observations of the RND group: the weighted intrinsic reward [N]"""
        self.update_counter += 1
        r, _ = self.raw_reward(new_state)
        r = self.reward_normalizer(r)
        self.weight = self.weight_at(self.update_counter)
        return r * self.weight

    @torch.no_grad()
    def collect_step(self, rewards_t, new_state):
        """steps 1 - 5: `rewards_t` [N] is the storage's slot of step t as the env kernel left it (r_ext + gamma V on time-outs); returns r_int"""
        r = self.intrinsic_reward(new_state)
        rewards_t += r
        return r

    def loss(self, state_rows):
        with torch.no_grad():
            s = self.state_normalizer(state_rows)
            t = self.target(s)
        return ((self.predictor(s) - t.detach()) ** 2).mean()


def make_optimizer(rnd):
    """THE separate optimiser: torch.optim.Adam's defaults on the predictor only"""
    return torch.optim.Adam(rnd.predictor.parameters(), lr=rnd.learning_rate)


def update_minibatch(rnd, optimizer, state_rows):
    """one RND step on the rows of a PPO mini-batch; returns the loss as a float"""
    loss = rnd.loss(state_rows)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()  # no clipping, a learning rate nobody moves
    return float(loss.detach())


def storage_state(storage, group):
    """the stored rows the predictor is trained on: o_t of the RND group, [T N, S]"""
    t = storage.observations if group == "policy" else storage.privileged_observations
    return t.reshape(-1, t.shape[-1])


# ---- cfg reading and refusals (no device, no env) ----------------------------------------------------------------------------------------
def _hidden(who, name, dims):
    dims = list(dims) if isinstance(dims, (list, tuple)) else None
    if dims is None or any(isinstance(d, bool) or not isinstance(d, numbers.Integral) for d in dims):
        raise ValueError(f"{who}: rnd {name} must be a list of layer widths, got {dims!r}")
    if -1 in dims:
        raise NotImplementedError(f"{who}: rnd {name}={dims} contains -1 (IsaacLab's \"as wide as the input\"): not implemented - spell the widths out")
    if any(d < 1 or d > MAX_WIDTH for d in dims) or len(dims) + 1 > MAX_LAYERS:
        raise ValueError(f"{who}: rnd {name}={dims}: at most {MAX_LAYERS} layers of width 1..{MAX_WIDTH} (the fused inference kernels and the HIP learner)")
    return tuple(int(d) for d in dims)


def check_rnd(who, rnd):
    """The `rnd=` dict of `Trainer` with its defaults filled in, or an error that says why it is refused."""
    if not isinstance(rnd, dict):
        raise TypeError(f"{who}: rnd must be a dict (weight, weight_schedule, reward_normalization, state_normalization, learning_rate, num_outputs, "
                        f"predictor_hidden_dims, target_hidden_dims, group), not {type(rnd).__name__}")
    unknown = sorted(set(rnd) - set(RND_KEYS))
    if unknown:
        raise ValueError(f"{who}: rnd has unknown keys {unknown} (known: {list(RND_KEYS)})")
    for k in ("weight", "predictor_hidden_dims", "target_hidden_dims"):
        if k not in rnd:
            raise ValueError(f"{who}: rnd needs {k!r}")
    w = rnd["weight"]
    if isinstance(w, bool) or not isinstance(w, numbers.Real) or not math.isfinite(w):
        raise ValueError(f"{who}: rnd weight must be a finite number, got {w!r}")
    lr = rnd.get("learning_rate", 1e-3)
    if isinstance(lr, bool) or not isinstance(lr, numbers.Real) or not math.isfinite(lr) or not lr > 0:
        raise ValueError(f"{who}: rnd learning_rate must be finite and > 0, got {lr!r}")
    k_out = rnd.get("num_outputs", 1)
    if isinstance(k_out, bool) or not isinstance(k_out, numbers.Integral) or not 1 <= k_out <= MAX_WIDTH:
        raise ValueError(f"{who}: rnd num_outputs must be 1..{MAX_WIDTH}, got {k_out!r}")
    group = rnd.get("group", "policy")
    if isinstance(group, (list, tuple)):
        if len(group) != 1:
            raise NotImplementedError(f"{who}: rnd group={list(group)}: the RND state is ONE observation group (no concatenation of groups is wired to the "
                                      "fused inference kernels)")
        group = group[0]
    if group not in ("policy", "critic"):
        raise ValueError(f"{who}: rnd group must be \"policy\" or \"critic\", not {group!r}")
    read_schedule(rnd.get("weight_schedule"))
    return dict(weight=float(w), weight_schedule=rnd.get("weight_schedule"), reward_normalization=bool(rnd.get("reward_normalization", False)),
                state_normalization=bool(rnd.get("state_normalization", False)), learning_rate=float(lr), num_outputs=int(k_out),
                predictor_hidden_dims=_hidden(who, "predictor_hidden_dims", rnd["predictor_hidden_dims"]),
                target_hidden_dims=_hidden(who, "target_hidden_dims", rnd["target_hidden_dims"]), group=group)


def check_rnd_trainer(rnd, rnn_type, symmetry, ppo_kw, normalization, group):
    """What `Trainer(rnd=...)` does not combine with is refused with a reason, never ignored - before the env is touched."""
    kw = check_rnd("Trainer", rnd)
    if rnn_type is not None:
        raise NotImplementedError("Trainer: rnd= with rnn_type= is not implemented: the recurrent collection loop and the recurrent learners walk the storage "
                                  "by env blocks and have no RND launches; drop rnd= or rnn_type=")
    if symmetry is not None or ppo_kw.get("mirror_loss") is not None:
        raise NotImplementedError("Trainer: rnd= with symmetry= / mirror_loss= is not implemented: whether the predictor trains on the mirrored copies of a "
                                  "mini-batch is not decided here; drop rnd= or symmetry=")
    if normalization:
        raise NotImplementedError("Trainer: rnd= with actor_obs_normalization / critic_obs_normalization is not implemented: the RND loop is the fused-act "
                                  "loop, which has no normalisation launches (RND's own state_normalization is part of rnd=); drop the flags or rnd=")
    if group is not None and getattr(group, "world_size", 1) > 1:
        raise NotImplementedError(f"Trainer: rnd= with a group of {group.world_size} ranks is not implemented: the predictor's gradients and the two "
                                  "normalisers' statistics are not exchanged between ranks; run one rank")
    return kw


def check_state_width(group, width):
    if width > MAX_WIDTH:
        raise ValueError(f"Trainer: the rnd state group {group!r} is {width} columns wide, the fused inference kernels and the HIP learner take at most "
                         f"{MAX_WIDTH} input columns: choose the other group or shorten its history_length")


def read_rnd_cfg(train_cfg: dict):
    """The `rnd=` dict of `Trainer` from a runner cfg (`algorithm.rnd_cfg` in IsaacLab's `RslRlRndCfg` field names, `obs_groups["rnd_state"]`), or None
    without an `rnd_cfg`.  Pure: no device, no env."""
    alg = dict(train_cfg.get("algorithm") or {})
    cfg = alg.get("rnd_cfg")
    if not cfg:
        return None
    if not isinstance(cfg, dict):
        cfg = {k: getattr(cfg, k) for k in RND_KEYS if hasattr(cfg, k)}
    cfg = dict(cfg)
    groups = dict(train_cfg.get("obs_groups") or {})
    sets = groups.get("rnd_state", ["policy"])
    sets = [sets] if isinstance(sets, str) else list(sets)
    if len(sets) != 1:
        raise NotImplementedError(f"stand-in runner: obs_groups['rnd_state'] = {sets}: the RND state is ONE observation group (no concatenation of groups is "
                                  "wired to the fused inference kernels)")
    unknown = sorted(set(cfg) - set(RND_KEYS) - {"class_name"})
    if unknown:
        raise NotImplementedError(f"stand-in runner: rnd_cfg fields {unknown} are not read here (known: {list(RND_KEYS[:-1])})")
    cfg.pop("class_name", None)
    cfg.pop("group", None)
    ws = cfg.get("weight_schedule")
    if ws is not None and not isinstance(ws, (dict, str)):
        cfg["weight_schedule"] = {k: getattr(ws, k) for k in ("mode", "initial_step", "final_step", "final_value") if hasattr(ws, k)}
    cfg.setdefault("weight", 0.0)
    cfg.setdefault("predictor_hidden_dims", [-1])  # (IsaacLab's defaults, refused below with the reason)
    cfg.setdefault("target_hidden_dims", [-1])
    return check_rnd("stand-in runner", dict(cfg, group=sets[0]))
