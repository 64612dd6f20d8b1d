"""The HIP-native PPO learner (`include/rl_ppo.h`, `csrc/rl_ppo.hip`): `PPO.update` of `robot_lab_amd/ppo.py` without torch autograd.

`ppo.PPO` stays the DEFINITION of the update rule; `HipPPO` evaluates the same rule - clipped surrogate,
clipped value loss, entropy bonus, KL-adaptive learning rate, gradient-norm clipping, Adam, the floor of std - with hand-written
gfx950 kernels on fp32 master parameters that live on the device.  One `update()` enqueues `num_learning_epochs x num_mini_batches`
mini-batches on the current stream and reads ONE small statistics block afterwards: no host synchronisation and no host decision
inside the update (the learning rate is a device word).  Opt-in: `Trainer(env, learner="hip")`, `tools/train_demo.py --learner hip`,
`RL_LEARNER=hip` for the runner behind the reference's `train.py`.

    alg = HipPPO(policy)                 # same keywords as ppo.PPO; copies the ActorCritic's parameters to the device (`load_from`)
    stats = alg.update(storage, gen)     # same statistics keys as PPO.update; draws the permutation as PPO.update does
    alg.push(actor, critic, std)         # new parameters into the inference kernels, device to device (rl_mlp_set_weights_device)
    alg.store_into(policy)               # back into the ActorCritic (checkpoints keep rsl_rl's state_dict layout)

`HipPPO(policy, symmetry=tables)` (a `symmetry.SymmetryTables`, as for `ppo.PPO`): symmetry data augmentation inside the update, the mirror
fused into the first layer's operand fetch and the loss head (`rl_ppo_set_symmetry`); `max_rows_per_minibatch` keeps counting stored rows.
`HipPPO(policy, symmetry=tables, mirror_loss=c, data_augmentation=True | False)`: rsl_rl's mirror loss on the same tables, as `ppo.PPO`
defines it (`rl_ppo_set_mirror_loss`); `update()` then returns `mirror_loss` too, read in the same one wait (`rl_ppo_stats_ex`).

`HipPPO(policy, obs_normalizers=(actor | None, critic | None))` (`obsnorm.ObsNormalizer` handles, the device half of the policy's
`actor_obs_normalizer` / `critic_obs_normalizer`): the storage given to `update()` holds RAW rows and the first layer's operand fetch
normalises them - behind the mirror, with the statistics the handles hold when the kernels run (`rl_ppo_set_obs_normalization`): the rule of
`ppo.PPO.update` on a raw batch, and what makes `symmetry=` and normalised observations go together.  Without the keyword a policy with
normalisers is fed matrices that were normalised before (`ppo.NormalizedBatch`).

`HipPPO(policy, group=g)` (a `dist.LearnerGroup`, or anything with `world_size`, `enabled` and an in-place `all_reduce_sum(tensor)`): rsl_rl's
multi-GPU contract.  The library holds no communicator: with an enabled group `update()` runs `rl_ppo_update_begin`, then per mini-batch
`rl_ppo_minibatch_local` -> `group.all_reduce_sum(wire)` -> `rl_ppo_minibatch_apply`, all on the current stream, and reads the one statistics
block afterwards.  The wire is the learner's flat gradient buffer adopted as a torch tensor, P gradient words and this rank's KL statistic in
word [P]: ONE collective per mini-batch carries both (the torch learner uses two).  `apply` divides by the world in fp32, as `LearnerGroup`
does.  Each rank draws its own permutation.  A disabled group (a world of one) or `None` takes the fused `rl_ppo_update`.

    alg.optimizer_state_dict()           # the layout of torch.optim.Adam(policy.parameters()).state_dict(): loads into ppo.PPO's optimizer
    alg.load_optimizer_state_dict(d)     # ... and back: a checkpoint written by either learner resumes the other
    alg.policy                           # the ActorCritic a checkpoint stores (refresh it with `store_into(alg.policy)` before reading it)

There is no CPU path and no fall-back to the torch learner: a missing library or an unsupported network raises."""
from __future__ import annotations

import ctypes as C
import math

from .capi import PPO_EXPORTS, PPO_LIB, Batch, Hyper, RlPpoError, load_ppo_library  # noqa: F401  (the binding of include/rl_ppo.h)

ACTIVATIONS = {"ELU": 0, "ReLU": 1, "Tanh": 2}
MAX_LAYERS, MAX_WIDTH = 8, 512


def _network(seq, name):
    """(dims, activation class name) of an nn.Sequential of Linear layers with one activation between them; anything else is refused."""
    from torch import nn

    mods = list(seq)
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    acts = [m for m in mods if not isinstance(m, nn.Linear)]
    if not lin or len(mods) != 2 * len(lin) - 1 or any(isinstance(m, nn.Linear) != (i % 2 == 0) for i, m in enumerate(mods)):
        raise ValueError(f"HipPPO: the {name} is not a Linear / activation / ... / Linear stack: unsupported network (use the torch learner, ppo.PPO)")
    kinds = {type(m).__name__ for m in acts}
    if len(kinds) > 1:
        raise ValueError(f"HipPPO: the {name} mixes activations {sorted(kinds)}: unsupported network (use the torch learner, ppo.PPO)")
    if any(m.bias is None for m in lin):
        raise ValueError(f"HipPPO: the {name} has a Linear layer without bias: unsupported network (use the torch learner, ppo.PPO)")
    return [lin[0].in_features] + [m.out_features for m in lin], (kinds.pop() if kinds else "ELU")


def parameter_shapes(actor_dims, critic_dims):
    """shapes of `ActorCritic.parameters()` (= the flat layout of include/rl_ppo.h): std, then W, b per actor layer, then the critic's"""
    shapes = [(actor_dims[-1],)]
    for dims in (actor_dims, critic_dims):
        for l in range(len(dims) - 1):
            shapes += [(dims[l + 1], dims[l]), (dims[l + 1],)]
    return shapes


def adam_state_dict(shapes, exp_avg, exp_avg_sq, step, lr):
    """`torch.optim.Adam(params, lr=lr).state_dict()` for parameters of `shapes`, from the flat moments, the common step count and the
    learning rate.  step == 0: no state, as an optimiser that has not stepped."""
    import torch

    group = torch.optim.Adam([torch.zeros(1)], lr=float(lr)).state_dict()["param_groups"][0]  # the defaults of THIS torch
    group["params"] = list(range(len(shapes)))
    state, o = {}, 0
    for i, shp in enumerate(shapes):
        n = math.prod(shp)
        if step > 0:
            state[i] = dict(step=torch.tensor(float(step), dtype=torch.float32), exp_avg=exp_avg[o:o + n].reshape(shp).clone(),
                            exp_avg_sq=exp_avg_sq[o:o + n].reshape(shp).clone())
        o += n
    if o != exp_avg.numel() or o != exp_avg_sq.numel():
        raise ValueError(f"adam_state_dict: the moments hold {exp_avg.numel()} / {exp_avg_sq.numel()} entries, the shapes {o}")
    return dict(state=state, param_groups=[group])


def adam_state_flat(d, shapes):
    """(exp_avg flat | None, exp_avg_sq flat | None, step, lr) of an Adam `state_dict()` over parameters of `shapes`; None moments: no state."""
    import torch

    groups = d["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(shapes):
        raise ValueError(f"optimizer state: expected one param group of {len(shapes)} parameters, got {[len(g['params']) for g in groups]}")
    g = groups[0]
    if tuple(g.get("betas", (0.9, 0.999))) != (0.9, 0.999) or g.get("eps", 1e-8) != 1e-8 or g.get("weight_decay", 0) or g.get("amsgrad") or g.get("maximize"):
        raise ValueError("optimizer state: the HIP learner implements torch.optim.Adam's defaults only (betas, eps, no weight decay / amsgrad / maximize)")
    state = d["state"]
    if not state:
        return None, None, 0, float(g["lr"])
    m1, m2, steps = [], [], set()
    for k, shp in zip(g["params"], shapes):
        e = state[k]
        if tuple(e["exp_avg"].shape) != tuple(shp) or tuple(e["exp_avg_sq"].shape) != tuple(shp):
            raise ValueError(f"optimizer state: parameter {k} has moments of shape {tuple(e['exp_avg'].shape)}, the learner's is {tuple(shp)}")
        m1.append(e["exp_avg"].reshape(-1))
        m2.append(e["exp_avg_sq"].reshape(-1))
        steps.add(int(float(e["step"])))
    if len(steps) != 1:
        raise ValueError(f"optimizer state: the parameters carry different step counts {sorted(steps)}: the HIP learner keeps one")
    return torch.cat(m1), torch.cat(m2), steps.pop(), float(g["lr"])


class _DevView:
    """`__cuda_array_interface__` holder: lets torch adopt the learner's wire without copying (the handle owns the memory: `close()` drops the view)"""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = dict(shape=(int(count),), typestr="<f4", data=(int(ptr), False), version=2, strides=None)


class HipPPO:
    """`ppo.PPO` on the HIP learner: same constructor keywords, same `update(storage, generator) -> dict`."""

    def __init__(self, policy, value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=5,
                 num_mini_batches=4, learning_rate=1.0e-3, schedule="adaptive", desired_kl=0.01, max_grad_norm=1.0, group=None,
                 max_rows_per_minibatch=None, lib_path: str | None = None, symmetry=None, mirror_loss=None, data_augmentation=True,
                 obs_normalizers=None, rnd=None):
        import torch

        from .ppo import check_mirror_loss

        # random network distillation: a robot_lab_amd.rnd_hip.HipRND, whose update is enqueued behind this learner's with the same permutation
        if rnd is not None:
            if not (callable(getattr(rnd, "update", None)) and callable(getattr(rnd, "stats", None)) and hasattr(rnd, "group")):
                raise TypeError(f"HipPPO: rnd must be a robot_lab_amd.rnd_hip.HipRND (or None), not {type(rnd).__name__}")
            if symmetry is not None or (group is not None and getattr(group, "enabled", False)):
                raise NotImplementedError("HipPPO: rnd= with symmetry= or an enabled group is not implemented (the predictor neither trains on mirrored copies "
                                          "nor exchanges gradients)")
        self.rnd = rnd

        if group is not None and not (isinstance(getattr(group, "world_size", None), int) and hasattr(group, "enabled") and callable(getattr(group, "all_reduce_sum", None))):
            raise NotImplementedError(f"HipPPO: group={type(group).__name__} has no world_size / enabled / all_reduce_sum(tensor): the HIP learner's multi-GPU "
                                      "path needs the SUM all-reduce of a robot_lab_amd.dist.LearnerGroup; any other gradient exchange is the torch learner, "
                                      "robot_lab_amd.ppo.PPO (Trainer(..., learner=\"torch\", group=...))")
        if group is not None and group.enabled and group.world_size < 1:
            raise ValueError(f"HipPPO: group.world_size={group.world_size} must be >= 1")
        if schedule not in ("adaptive", "fixed"):
            raise ValueError(f"HipPPO: unknown schedule {schedule!r} (\"adaptive\" or \"fixed\")")
        self._torch = torch
        self.handle = None
        adims, aact = _network(policy.actor, "actor")
        cdims, cact = _network(policy.critic, "critic")
        std = getattr(policy, "std", None)
        if std is None or getattr(policy, "noise_std_type", "scalar") != "scalar":
            raise ValueError("HipPPO: noise_std_type=\"log\" (or a policy without a `std` parameter) is unsupported: the HIP learner implements the scalar std only")
        if len(adims) != len(cdims):
            raise ValueError(f"HipPPO: actor and critic differ in depth ({len(adims) - 1} / {len(cdims) - 1} layers): unsupported network (use the torch learner)")
        if aact != cact or aact != "ELU":
            raise ValueError(f"HipPPO: unsupported activation {aact} / {cact}: the HIP learner implements ELU only (use the torch learner, ppo.PPO)")
        if len(adims) - 1 > MAX_LAYERS or max(adims + cdims) > MAX_WIDTH:
            raise ValueError(f"HipPPO: unsupported network: at most {MAX_LAYERS} layers of width <= {MAX_WIDTH} (got actor {adims}, critic {cdims}); use the torch learner")
        if tuple(std.shape) != (adims[-1],):
            raise ValueError("HipPPO: std must have one entry per action")
        if desired_kl is not None and not desired_kl > 0:
            raise ValueError(f"HipPPO: desired_kl={desired_kl!r} is unsupported: a positive target, or None for no KL-adaptive learning rate")
        if std.device.type != "cuda" or any(p.device != std.device for p in policy.parameters()):
            raise ValueError(f"HipPPO: the policy must live on one CUDA device (std is on {std.device}): the HIP learner has no CPU path - "
                             "move it with policy.to(\"cuda:0\") or use the torch learner, ppo.PPO")
        if symmetry is not None:
            from .symmetry import SymmetryTables

            if not isinstance(symmetry, SymmetryTables):
                raise TypeError(f"HipPPO: symmetry must be a robot_lab_amd.symmetry.SymmetryTables (or None), not {type(symmetry).__name__}")
            symmetry.check_widths(adims[0], cdims[0], adims[-1])
        self.symmetry = symmetry
        self.obs_normalizers = self._check_normalizers(policy, obs_normalizers, (adims[0], cdims[0]), std.device)  # (kept: the kernels read their memory)
        self._mirror = check_mirror_loss("HipPPO", symmetry, mirror_loss, data_augmentation)  # what the handle is given at its creation
        self.mirror_loss, self.data_augmentation = None, True  # what the handle HAS (set_mirror_loss)
        self.lib = load_ppo_library(lib_path)
        self.actor_dims, self.critic_dims, self.n_layers = adims, cdims, len(adims) - 1
        self.value_loss_coef, self.use_clipped_value_loss, self.clip_param, self.entropy_coef = value_loss_coef, use_clipped_value_loss, clip_param, entropy_coef
        self.num_learning_epochs, self.num_mini_batches = num_learning_epochs, num_mini_batches
        self.learning_rate, self.schedule, self.desired_kl, self.max_grad_norm = learning_rate, schedule, desired_kl, max_grad_norm
        self.group = group if group is not None and group.enabled else None  # a world of one: the fused rl_ppo_update, no collective
        self._wire = None
        self._opt_pending = None
        self.policy = policy  # the module a checkpoint stores (`store_into(alg.policy)` refreshes it)
        self.device = std.device
        self.max_rows = int(max_rows_per_minibatch or 0)
        self._policy = policy
        self.last_grad_norm = float("nan")
        if self.max_rows:
            self._create(self.max_rows)

    # -- handle ---------------------------------------------------------------------------------------------------------------------
    def _hyper(self):
        return Hyper(learning_rate=float(self.learning_rate), desired_kl=float(self.desired_kl) if self.desired_kl is not None else 0.0,
                     value_loss_coef=self.value_loss_coef, clip_param=self.clip_param, entropy_coef=self.entropy_coef, max_grad_norm=self.max_grad_norm,
                     use_clipped_value_loss=int(bool(self.use_clipped_value_loss)), num_learning_epochs=self.num_learning_epochs,
                     num_mini_batches=self.num_mini_batches,
                     schedule=1 if self.schedule == "adaptive" and self.desired_kl is not None else 0, std_type=0)  # (ppo.py: adaptive needs a target)

    def _check(self, rc):
        if rc != 0:
            raise RlPpoError((self.lib.rl_ppo_last_error() or b"").decode())

    def _create(self, max_rows):
        """(the handle is sized by the largest mini-batch: created at the first update unless `max_rows_per_minibatch` was given)"""
        hp, n = self._hyper(), self.n_layers
        handle = C.c_void_p()
        rc = self.lib.rl_ppo_create((C.c_int32 * (n + 1))(*self.actor_dims), (C.c_int32 * (n + 1))(*self.critic_dims), n, ACTIVATIONS["ELU"], C.byref(hp),
                                    int(max_rows), self.device.index or 0, C.byref(handle))
        self._check(rc)
        self.handle, self.max_rows = handle, int(max_rows)
        try:
            if self.symmetry is not None:
                self.set_symmetry(self.symmetry)
                if self._mirror[0] is not None:
                    self.set_mirror_loss(*self._mirror)
            if self.obs_normalizers is not None:
                self._set_obs_normalization(self.obs_normalizers)
            if self.group is not None:
                self._set_world(self.group.world_size)
        except Exception:
            self.close()  # never a learner that quietly runs without the symmetry, the normalisation or the world it was asked for
            raise
        self.num_parameters = int(self.lib.rl_ppo_num_parameters(self.handle))
        if self._opt_pending is not None:
            d, self._opt_pending = self._opt_pending, None
            self.load_optimizer_state_dict(d)
        if self._policy is not None:
            self.load_from(self._policy)
            self._policy = None

    def set_symmetry(self, tables):
        """`rl_ppo_set_symmetry`: once per handle, before its first mini-batch (the constructor's `symmetry=` does it at handle creation)."""
        import numpy as np

        if self.handle is None:
            raise RlPpoError("HipPPO.set_symmetry before the handle exists: pass symmetry= to the constructor")
        ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        keep, args = [], []
        for t in (tables.obs, tables.critic, tables.act):
            if t is None:
                args += [None, None]
                continue
            perm, sign = np.ascontiguousarray(t[0], dtype=np.int32), np.ascontiguousarray(t[1], dtype=np.float32)
            keep += [perm, sign]
            args += [perm.ctypes.data_as(ip), sign.ctypes.data_as(fp)]
        self._check(self.lib.rl_ppo_set_symmetry(self.handle, int(tables.n_sym), *args))
        self.symmetry = tables

    def set_mirror_loss(self, coeff, data_augmentation=True):
        """`rl_ppo_set_mirror_loss`: once per handle, after the symmetry and before the first mini-batch (the constructor's `mirror_loss=`
        does it at handle creation).  The library checks for itself; a refused call leaves the learner as it was."""
        if self.handle is None:
            raise RlPpoError("HipPPO.set_mirror_loss before the handle exists: pass mirror_loss= to the constructor")
        self._check(self.lib.rl_ppo_set_mirror_loss(self.handle, float(coeff), int(bool(data_augmentation))))
        self.mirror_loss, self.data_augmentation = float(coeff), bool(data_augmentation)

    @staticmethod
    def _check_normalizers(policy, handles, widths, device):
        """`obs_normalizers=` as a pair (actor handle | None, critic handle | None), or None; a ValueError says why a pair does not fit"""
        if handles is None:
            return None
        from torch import nn

        handles = tuple(handles)
        if len(handles) != 2 or all(h is None for h in handles):
            raise ValueError("HipPPO: obs_normalizers must be a pair (actor handle | None, critic handle | None) with at least one handle "
                             "(no normalisation in the learner: drop the keyword)")
        for name, h, width in zip(("actor", "critic"), handles, widths):
            module = getattr(policy, f"{name}_obs_normalizer", None)
            identity = module is None or isinstance(module, nn.Identity)
            if h is None:
                if not identity:
                    raise ValueError(f"HipPPO: obs_normalizers has no handle for the {name}, but the policy's {name}_obs_normalizer is a "
                                     f"{type(module).__name__}: the learner would train on raw rows a policy that normalises them")
                continue
            if identity:
                raise ValueError(f"HipPPO: obs_normalizers has a handle for the {name}, but the policy's {name}_obs_normalizer is nn.Identity: the "
                                 f"policy was built without {name}_obs_normalization")
            if int(h.dim) != width:
                raise ValueError(f"HipPPO: the {name}'s normaliser is {h.dim} columns wide, the network's input {width}")
            if (h.device.type, h.device.index or 0) != (device.type, device.index or 0):  # ("cuda" is cuda:0, as obsnorm.py creates it)
                raise ValueError(f"HipPPO: the {name}'s normaliser lives on {h.device}, the policy on {device}")
        return handles

    def _set_obs_normalization(self, handles):
        """`rl_ppo_set_obs_normalization`: once per handle, before its first mini-batch (the constructor's `obs_normalizers=` at handle creation)"""
        args = []
        for h in handles:
            mean, std, eps = h.device_pointers() if h is not None else (None, None, 0.0)
            args += [C.c_void_p(mean), C.c_void_p(std), float(eps)]
        self._check(self.lib.rl_ppo_set_obs_normalization(self.handle, *args))

    def _set_world(self, world_size):
        """`rl_ppo_set_world` + the wire adopted as a torch tensor (P + 1 floats of the learner's gradient buffer, no copy)"""
        self._check(self.lib.rl_ppo_set_world(self.handle, int(world_size)))
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self.lib.rl_ppo_wire(self.handle, C.byref(ptr), C.byref(cnt)))
        self._wire = self._torch.as_tensor(_DevView(ptr.value, cnt.value), device=self.device)

    def _need(self, rows):
        if self.handle is None:
            self._create(rows)
        elif rows > self.max_rows:
            raise RlPpoError(f"mini-batch of {rows} rows > max_rows_per_minibatch {self.max_rows} the learner was created with")

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _layers(self, policy):
        nn = self._torch.nn
        la, lc = [m for m in policy.actor if isinstance(m, nn.Linear)], [m for m in policy.critic if isinstance(m, nn.Linear)]
        if [la[0].in_features] + [m.out_features for m in la] != self.actor_dims or [lc[0].in_features] + [m.out_features for m in lc] != self.critic_dims:
            raise ValueError("HipPPO: the policy's layer shapes differ from the learner's")
        return la, lc

    def _arrays(self, policy):
        la, lc = self._layers(policy)
        ts = []

        def arr(params):
            out = []
            for t in params:
                t = t.detach()
                if t.dtype != self._torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"HipPPO: parameters must be contiguous float32 tensors on {self.device}")
                ts.append(t)
                out.append(t.data_ptr())
            return (C.c_void_p * len(out))(*out)

        return arr(m.weight for m in la), arr(m.bias for m in la), arr(m.weight for m in lc), arr(m.bias for m in lc), policy.std.detach()

    def load_from(self, policy):
        """The ActorCritic's parameters become the learner's master parameters (device-to-device).  Adam's moments and step are kept."""
        if self.handle is None:
            self._policy = policy
            return
        aw, ab, cw, cb, std = self._arrays(policy)
        self._check(self.lib.rl_ppo_set_parameters(self.handle, aw, ab, cw, cb, C.c_void_p(std.data_ptr()), self._stream()))

    def store_into(self, policy):
        """The master parameters back into an ActorCritic (for `state_dict()`: rsl_rl's checkpoint layout)."""
        if self.handle is None:
            if self._policy is not None and self._policy is not policy:
                policy.load_state_dict(self._policy.state_dict())
            return policy
        aw, ab, cw, cb, std = self._arrays(policy)
        self._check(self.lib.rl_ppo_get_parameters(self.handle, aw, ab, cw, cb, C.c_void_p(std.data_ptr()), self._stream()))
        return policy

    def push(self, actor, critic, std_tensor):
        """The master parameters into the inference kernels' images (`MlpPolicy`) and the sampling kernel's std tensor, on the current
        stream, without the host: `rl_mlp_set_weights_device` reads the flat parameter buffer in place."""
        if self.handle is None:
            raise RlPpoError("HipPPO.push before the first update: nothing to push")
        n = self.n_layers
        aw, ab, cw, cb = ((C.c_void_p * n)() for _ in range(4))
        sd = C.c_void_p()
        self._check(self.lib.rl_ppo_parameter_pointers(self.handle, aw, ab, cw, cb, C.byref(sd)))
        actor.set_weights_device([int(x) for x in aw], [int(x) for x in ab])
        critic.set_weights_device([int(x) for x in cw], [int(x) for x in cb])
        if std_tensor.dtype != self._torch.float32 or not std_tensor.is_contiguous() or std_tensor.numel() != self.actor_dims[-1]:
            raise ValueError("HipPPO.push: std_tensor must be a contiguous float32 tensor with one entry per action")
        self._check(self.lib.rl_ppo_get_parameters(self.handle, None, None, None, None, C.c_void_p(std_tensor.data_ptr()), self._stream()))

    def flat(self, which="parameters"):
        """A copy of a flat device buffer (`ActorCritic.parameters()` order): "parameters", "gradients", "exp_avg", "exp_avg_sq"."""
        if self.handle is None:
            raise RlPpoError("HipPPO.flat before the handle exists (pass max_rows_per_minibatch or run an update)")
        out = self._torch.empty(self.num_parameters, device=self.device, dtype=self._torch.float32)
        self._check(self.lib.rl_ppo_get_flat(self.handle, ["parameters", "gradients", "exp_avg", "exp_avg_sq"].index(which), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- optimiser state (checkpoints) -------------------------------------------------------------------------------------------
    def optimizer_state_dict(self):
        """The layout of `torch.optim.Adam(policy.parameters()).state_dict()`: per-parameter `step`, `exp_avg`, `exp_avg_sq` in
        `ActorCritic.parameters()` order and `param_groups[0]["lr"]`.  One wait of the current stream."""
        shapes = parameter_shapes(self.actor_dims, self.critic_dims)
        if self.handle is None:  # no update yet: what was loaded, or an optimiser that has not stepped
            zeros = self._torch.zeros(sum(math.prod(shp) for shp in shapes))
            return self._opt_pending if self._opt_pending is not None else adam_state_dict(shapes, zeros, zeros, 0, self.learning_rate)
        lr, step = C.c_double(), C.c_int64()
        self._check(self.lib.rl_ppo_get_optimizer(self.handle, C.byref(lr), C.byref(step), self._stream()))
        return adam_state_dict(shapes, self.flat("exp_avg"), self.flat("exp_avg_sq"), step.value, lr.value)

    def load_optimizer_state_dict(self, d):
        """An Adam `state_dict()` of this layout - written by this learner or by `ppo.PPO`'s optimizer - becomes the moments, the step counter and
        the learning-rate word (stream-ordered).  A state without entries (an optimiser that never stepped) zeroes the moments."""
        torch = self._torch
        m1, m2, step, lr = adam_state_flat(d, parameter_shapes(self.actor_dims, self.critic_dims))
        if self.handle is None:
            self._opt_pending = d
            self.learning_rate = lr
            return
        for which, m in ((2, m1), (3, m2)):
            m = torch.zeros(self.num_parameters, device=self.device) if m is None else m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.numel() != self.num_parameters:
                raise ValueError(f"optimizer state: {m.numel()} moment entries, the learner has {self.num_parameters} parameters")
            self._check(self.lib.rl_ppo_set_flat(self.handle, which, C.c_void_p(m.data_ptr()), self._stream()))  # (on torch's current stream: a temporary `m` is safe)
        self._check(self.lib.rl_ppo_set_optimizer(self.handle, lr, step, self._stream()))
        self.learning_rate = lr

    # -- the update -----------------------------------------------------------------------------------------------------------------
    def _batch(self, storage):
        torch = self._torch
        T, N = storage.num_transitions_per_env, storage.num_envs
        keep = []

        def ptr(t, width):
            t = t.reshape(T * N, -1)
            if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                t = t.to(device=self.device, dtype=torch.float32).contiguous()
            if t.shape[1] != width:
                raise ValueError(f"HipPPO: storage tensor of width {t.shape[1]}, expected {width}")
            keep.append(t)
            return t.data_ptr()

        A = self.actor_dims[-1]
        b = Batch(observations=ptr(storage.observations, self.actor_dims[0]), privileged_observations=ptr(storage.privileged_observations, self.critic_dims[0]),
                  actions=ptr(storage.actions, A), values=ptr(storage.values, 1), returns=ptr(storage.returns, 1), advantages=ptr(storage.advantages, 1),
                  actions_log_prob=ptr(storage.actions_log_prob, 1), mu=ptr(storage.mu, A), sigma=ptr(storage.sigma, A))
        return b, keep, T * N

    def minibatch_grad(self, storage, idx):
        """Forward, loss head and backward on the rows `idx` (int64 device tensor); returns the flat gradient.  No optimiser step."""
        b, keep, T_N = self._batch(storage)
        idx = idx.to(device=self.device, dtype=self._torch.int64).contiguous()
        if idx.numel() < 1 or int(idx.min()) < 0 or int(idx.max()) >= T_N:
            raise ValueError("HipPPO.minibatch_grad: idx must hold row numbers of the batch")
        self._need(idx.numel())
        self._check(self.lib.rl_ppo_minibatch_grad(self.handle, C.byref(b), C.c_void_p(idx.data_ptr()), idx.numel(), self._stream()))
        return self.flat("gradients")

    def update(self, storage, generator=None, perm=None) -> dict:
        """`PPO.update`: one permutation per update (drawn as `PPO.update` draws it unless `perm` is given), walked once per epoch."""
        torch = self._torch
        b, keep, B = self._batch(storage)
        if perm is None:
            perm = torch.randperm(B, device=self.device, generator=generator)
        else:  # the caller's rows (a test stepping one mini-batch at a time): checked, they index device memory
            if perm.numel() < self.num_mini_batches or perm.numel() > B or int(perm.min()) < 0 or int(perm.max()) >= B:
                raise ValueError("HipPPO.update: perm must hold between num_mini_batches and T * N row numbers of the batch")
        perm = perm.to(device=self.device, dtype=torch.int64).contiguous()
        rows = perm.numel()
        self._need(rows // self.num_mini_batches)
        if self.group is None:
            self._check(self.lib.rl_ppo_update(self.handle, C.byref(b), C.c_void_p(perm.data_ptr()), rows, self._stream()))
        else:  # the same sequence with the group's collective between the gradient and the step of every mini-batch; nothing waits on the host
            mb, stream = rows // self.num_mini_batches, self._stream()
            self._check(self.lib.rl_ppo_update_begin(self.handle, stream))
            for _ in range(self.num_learning_epochs):
                for i in range(self.num_mini_batches):
                    self._check(self.lib.rl_ppo_minibatch_local(self.handle, C.byref(b), C.c_void_p(perm.data_ptr() + 8 * i * mb), mb, stream))
                    try:
                        self.group.all_reduce_sum(self._wire)
                    except Exception as e:
                        # the gradient of this mini-batch waits for a step that will not come, and the other ranks are past it: fail-stop
                        self.close()
                        raise RlPpoError(f"HipPPO.update: the group's all_reduce_sum failed in mini-batch {i} ({type(e).__name__}: {e}); the learner's "
                                         "replicas can no longer be in step, so this learner is CLOSED - build a new one and load the last checkpoint") from e
                    self._check(self.lib.rl_ppo_minibatch_apply(self.handle, stream))
        if self.rnd is not None:
            # THE RULE takes the predictor's step right behind the PPO step of each mini-batch; the two touch disjoint state (the target and the
            # normaliser's statistics are constants of the update), so all PPO mini-batches followed by all RND mini-batches over the SAME perm give
            # the same bits - and the PPO half is the launch sequence of a learner without rnd=
            from .rnd import storage_state

            self.rnd.update(storage_state(storage, self.rnd.group), perm, checked=True)
        # the one wait of the update (keeps `keep` / `perm` alive until then)
        if self.mirror_loss is None:
            out = (C.c_double * 8)()
            self._check(self.lib.rl_ppo_stats(self.handle, out, self._stream()))
        else:
            out = (C.c_double * 9)()
            self._check(self.lib.rl_ppo_stats_ex(self.handle, out, 9, self._stream()))
        self.learning_rate, self.last_grad_norm = float(out[4]), float(out[5])
        res = dict(value_loss=float(out[0]), surrogate_loss=float(out[1]), entropy=float(out[2]), kl=float(out[3]))
        if self.mirror_loss is not None:
            res["mirror_loss"] = float(out[8])
        if self.rnd is not None:
            res.update(self.rnd.stats())  # (the stream has been waited for: a small copy)
        res["learning_rate"] = self.learning_rate
        return res

    def close(self):
        self._wire = None  # (a view of the handle's memory)
        if getattr(self, "handle", None):
            self.lib.rl_ppo_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        from .ppo import mirror_repr

        sym = f", symmetry={self.symmetry!r}{mirror_repr(self)}" if self.symmetry is not None else ""
        if self.obs_normalizers is not None:
            sym += f", obs_normalizers={[n for n, h in zip(('actor', 'critic'), self.obs_normalizers) if h is not None]}"
        return f"HipPPO(actor={self.actor_dims}, critic={self.critic_dims}, schedule={self.schedule!r}, lr={self.learning_rate:g}{sym}, librl_ppo_hip)"
