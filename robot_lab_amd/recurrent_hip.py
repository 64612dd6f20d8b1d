"""The HIP-native recurrent PPO learner (`include/rl_bptt.h`, `csrc/learner/rl_bptt.inl` inside librl_ppo_hip.so): `RecurrentPPO.update` of
`robot_lab_amd/recurrent.py` - back-propagation through time - without torch autograd.

`recurrent.RecurrentPPO` stays the DEFINITION of the rule; `HipRecurrentPPO` evaluates the same rule - contiguous blocks of envs over all T steps,
the recurrence from the saved state of step 0 with the input state zeroed behind a done, the PPO loss with the KL-adaptive learning rate,
gradient-norm clipping, Adam, the floor of std - on fp32 master parameters that live on the device.  One `update()` enqueues every block on the
current stream and reads ONE small statistics block afterwards.

    alg = HipRecurrentPPO(policy, **ppo_kw)      # same keywords as recurrent.RecurrentPPO; the policy is an ActorCriticRecurrent on a GPU
    stats = alg.update(batch)                    # batch: a recurrent.RecurrentBatch; the keys of RecurrentPPO.update
    alg.push(cell_a, cell_c, actor, critic, std) # the master parameters into the collection's kernels, device to device, current stream
    alg.sync_policy()                            # back into the module (checkpoints keep rsl_rl's state_dict layout)
    alg.optimizer_state_dict()                   # the layout of torch.optim.Adam(policy.parameters()).state_dict(): either learner resumes the other

The handle is sized by the storage (T steps x N envs): it is created at the first `update` / `block_grad` / `forward`, or at construction with
`num_steps=` and `num_envs=`.  There is no CPU path and no fall-back to the torch learner: a missing library or an unsupported network raises."""
from __future__ import annotations

import ctypes as C
import math

from .capi import PPO_LIB, Hyper, RlPpoError
from .ppo_hip import ACTIVATIONS, MAX_LAYERS, MAX_WIDTH, _network, adam_state_dict, adam_state_flat

BPTT_EXPORTS = ["rl_bptt_create", "rl_bptt_destroy", "rl_bptt_last_error", "rl_bptt_num_parameters", "rl_bptt_set_parameters", "rl_bptt_get_parameters",
                "rl_bptt_parameter_pointers", "rl_bptt_get_flat", "rl_bptt_set_flat", "rl_bptt_get_optimizer", "rl_bptt_set_optimizer", "rl_bptt_block_grad",
                "rl_bptt_forward", "rl_bptt_update", "rl_bptt_stats"]
FLATS = ["parameters", "gradients", "exp_avg", "exp_avg_sq"]
_lib = None


class RlBpttError(RlPpoError):
    pass


class BpttBatch(C.Structure):
    """include/rl_bptt.h `rl_bptt_batch`"""
    _fields_ = [(n, C.c_void_p) for n in ("observations", "privileged_observations", "actions", "values", "returns", "advantages", "actions_log_prob", "mu",
                                          "sigma", "dones", "h0_a", "c0_a", "h0_c", "c0_c")]


def load_bptt_library(path: str | None = None) -> C.CDLL:
    """the learner library (the PPO learner's: the recurrent learner shares its kernels) with the prototypes of include/rl_bptt.h"""
    global _lib
    import os

    path = path or os.environ.get("RL_PPO_LIB") or PPO_LIB
    if _lib is not None and path == PPO_LIB:
        return _lib
    if not os.path.isfile(path):
        raise RlBpttError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (the HIP learner has no CPU fallback)")
    lib = C.CDLL(path)
    if not hasattr(lib, "rl_bptt_create"):
        raise RlBpttError(f"{path} has no rl_bptt_create: this learner library predates the recurrent learner, rebuild it")
    vp, pp, i32 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int32
    lib.rl_bptt_create.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), i32, i32, C.POINTER(Hyper), i32, i32, i32, pp]
    lib.rl_bptt_destroy.argtypes = [vp]
    lib.rl_bptt_last_error.restype = C.c_char_p
    lib.rl_bptt_num_parameters.argtypes = [vp]
    lib.rl_bptt_num_parameters.restype = C.c_int64
    lib.rl_bptt_set_parameters.argtypes = [vp, pp, pp, pp, pp, pp, pp, vp, vp]
    lib.rl_bptt_get_parameters.argtypes = [vp, pp, pp, pp, pp, pp, pp, vp, vp]
    lib.rl_bptt_parameter_pointers.argtypes = [vp, pp, pp, pp, pp, pp, pp, pp]
    lib.rl_bptt_get_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_bptt_set_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_bptt_get_optimizer.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), vp]
    lib.rl_bptt_set_optimizer.argtypes = [vp, C.c_double, C.c_int64, vp]
    lib.rl_bptt_block_grad.argtypes = [vp, C.POINTER(BpttBatch), i32, vp]
    lib.rl_bptt_forward.argtypes = [vp, C.POINTER(BpttBatch), i32, vp, vp, vp]
    lib.rl_bptt_update.argtypes = [vp, C.POINTER(BpttBatch), vp]
    lib.rl_bptt_stats.argtypes = [vp, C.POINTER(C.c_double), vp]
    if path == PPO_LIB:
        _lib = lib
    return lib


def recurrent_parameter_shapes(obs_dim, critic_obs_dim, hidden, actor_dims, critic_dims):
    """shapes of `ActorCriticRecurrent.parameters()` (= the flat layout of include/rl_bptt.h): std; weight_ih, weight_hh, bias_ih, bias_hh of
    memory_a, then of memory_c; W, b per actor layer, then the critic's"""
    H4 = 4 * hidden
    shapes = [(actor_dims[-1],)]
    for D in (obs_dim, critic_obs_dim):
        shapes += [(H4, D), (H4, hidden), (H4,), (H4,)]
    for dims in (actor_dims, critic_dims):
        for l in range(len(dims) - 1):
            shapes += [(dims[l + 1], dims[l]), (dims[l + 1],)]
    return shapes


class HipRecurrentPPO:
    """`recurrent.RecurrentPPO` on the HIP learner: same constructor keywords, same `update(batch) -> dict`."""

    def __init__(self, policy, value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=5,
                 num_mini_batches=4, learning_rate=1.0e-3, schedule="adaptive", desired_kl=0.01, max_grad_norm=1.0, group=None, symmetry=None,
                 mirror_loss=None, data_augmentation=True, num_steps=None, num_envs=None, lib_path: str | None = None):
        import torch

        from .recurrent import ActorCriticRecurrent

        for refused, v, why in (("symmetry", symmetry, "mirroring an observation sequence through the memory is not defined here"),
                                ("mirror_loss", mirror_loss, "it needs symmetry="), ("group", group, "the ranks' block order and state exchange are not decided")):
            if v is not None and not (refused == "group" and getattr(v, "world_size", 1) <= 1):
                raise NotImplementedError(f"HipRecurrentPPO: {refused}= with a recurrent policy is not implemented: {why}")
        if not isinstance(policy, ActorCriticRecurrent):
            raise TypeError(f"HipRecurrentPPO: policy must be an ActorCriticRecurrent, not {type(policy).__name__}")
        if schedule not in ("adaptive", "fixed"):
            raise ValueError(f"HipRecurrentPPO: unknown schedule {schedule!r} (\"adaptive\" or \"fixed\")")
        if desired_kl is not None and not desired_kl > 0:
            raise ValueError(f"HipRecurrentPPO: desired_kl={desired_kl!r} is unsupported: a positive target, or None for no KL-adaptive learning rate")
        self._torch = torch
        self.handle = None
        adims, aact = _network(policy.actor, "actor")
        cdims, cact = _network(policy.critic, "critic")
        if len(adims) != len(cdims):
            raise ValueError(f"HipRecurrentPPO: actor and critic heads differ in depth ({len(adims) - 1} / {len(cdims) - 1} layers): unsupported network (use the torch learner)")
        if aact != cact or aact != "ELU":
            raise ValueError(f"HipRecurrentPPO: unsupported activation {aact} / {cact}: the HIP learner implements ELU only (use the torch learner, recurrent.RecurrentPPO)")
        ra, rc = policy.memory_a.rnn, policy.memory_c.rnn
        H = int(policy.rnn_hidden_dim)
        for name, r in (("memory_a", ra), ("memory_c", rc)):
            if not isinstance(r, torch.nn.LSTM) or r.num_layers != 1 or r.bidirectional or not r.bias or r.hidden_size != H or getattr(r, "proj_size", 0):
                raise NotImplementedError(f"HipRecurrentPPO: {name} is not a single-layer, one-directional nn.LSTM of hidden size {H} with biases: GRU and stacked "
                                          "layers are not implemented (use the torch learner)")
        widths = [ra.input_size, rc.input_size, H] + adims + cdims
        if len(adims) - 1 > MAX_LAYERS or max(widths) > MAX_WIDTH or adims[0] != H or cdims[0] != H:
            raise ValueError(f"HipRecurrentPPO: unsupported network: heads of at most {MAX_LAYERS} layers behind a hidden state of {H}, every width <= {MAX_WIDTH} "
                             f"(got obs {ra.input_size} / {rc.input_size}, actor {adims}, critic {cdims}); use the torch learner")
        std = policy.std
        if std.device.type != "cuda" or any(p.device != std.device for p in policy.parameters()):
            raise ValueError(f"HipRecurrentPPO: the policy must live on one CUDA device (std is on {std.device}): the HIP learner has no CPU path - "
                             "move it with policy.to(\"cuda:0\") or use the torch learner, recurrent.RecurrentPPO")
        self.lib = load_bptt_library(lib_path)
        self.policy, self.device = policy, std.device
        self.obs_dim, self.critic_obs_dim, self.hidden = int(ra.input_size), int(rc.input_size), H
        self.actor_dims, self.critic_dims, self.n_layers = adims, cdims, len(adims) - 1
        self.value_loss_coef, self.use_clipped_value_loss, self.clip_param, self.entropy_coef = value_loss_coef, use_clipped_value_loss, clip_param, entropy_coef
        self.num_learning_epochs, self.num_mini_batches = int(num_learning_epochs), int(num_mini_batches)
        self.learning_rate, self.schedule, self.desired_kl, self.max_grad_norm = learning_rate, schedule, desired_kl, max_grad_norm
        self.last_grad_norm = float("nan")
        self.T = self.N = None
        self._opt_pending = None
        if (num_steps is None) != (num_envs is None):
            raise ValueError("HipRecurrentPPO: num_steps= and num_envs= size the handle together: give both or neither")
        if num_steps is not None:
            self._create(int(num_steps), int(num_envs))

    # -- handle ---------------------------------------------------------------------------------------------------------------------
    def shapes(self):
        return recurrent_parameter_shapes(self.obs_dim, self.critic_obs_dim, self.hidden, self.actor_dims, self.critic_dims)

    def _hyper(self):
        return Hyper(learning_rate=float(self.learning_rate), desired_kl=float(self.desired_kl) if self.desired_kl is not None else 0.0,
                     value_loss_coef=self.value_loss_coef, clip_param=self.clip_param, entropy_coef=self.entropy_coef, max_grad_norm=self.max_grad_norm,
                     use_clipped_value_loss=int(bool(self.use_clipped_value_loss)), num_learning_epochs=self.num_learning_epochs,
                     num_mini_batches=self.num_mini_batches,
                     schedule=1 if self.schedule == "adaptive" and self.desired_kl is not None else 0, std_type=0)

    def _check(self, rc):
        if rc != 0:
            raise RlBpttError((self.lib.rl_bptt_last_error() or b"").decode())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _create(self, T, N):
        hp, n = self._hyper(), self.n_layers
        handle = C.c_void_p()
        rc = self.lib.rl_bptt_create(self.obs_dim, self.critic_obs_dim, self.hidden, (C.c_int32 * (n + 1))(*self.actor_dims),
                                     (C.c_int32 * (n + 1))(*self.critic_dims), n, ACTIVATIONS["ELU"], C.byref(hp), int(T), int(N), self.device.index or 0,
                                     C.byref(handle))
        self._check(rc)
        self.handle, self.T, self.N = handle, int(T), int(N)
        self.num_parameters = int(self.lib.rl_bptt_num_parameters(self.handle))
        self.load_from(self.policy)
        if self._opt_pending is not None:
            d, self._opt_pending = self._opt_pending, None
            self.load_optimizer_state_dict(d)

    def _need(self, T, N):
        if self.handle is None:
            self._create(T, N)
        elif (T, N) != (self.T, self.N):
            raise RlBpttError(f"a storage of {T} steps x {N} envs, the learner was created for {self.T} x {self.N}")

    def _arrays(self, policy):
        """the seven ctypes arguments of rl_bptt_set_parameters / get_parameters (+ the tensors, kept alive by the caller)"""
        nn = self._torch.nn
        la, lc = [m for m in policy.actor if isinstance(m, nn.Linear)], [m for m in policy.critic if isinstance(m, nn.Linear)]
        if [la[0].in_features] + [m.out_features for m in la] != self.actor_dims or [lc[0].in_features] + [m.out_features for m in lc] != self.critic_dims:
            raise ValueError("HipRecurrentPPO: the policy's layer shapes differ from the learner's")
        keep = []

        def arr(params):
            out = []
            for t in params:
                t = t.detach()
                if t.dtype != self._torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"HipRecurrentPPO: parameters must be contiguous float32 tensors on {self.device}")
                keep.append(t)
                out.append(t.data_ptr())
            return (C.c_void_p * len(out))(*out)

        lstm = lambda r: arr((r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0))  # noqa: E731
        ra, rc = policy.memory_a.rnn, policy.memory_c.rnn
        if tuple(ra.weight_ih_l0.shape) != (4 * self.hidden, self.obs_dim) or tuple(rc.weight_ih_l0.shape) != (4 * self.hidden, self.critic_obs_dim):
            raise ValueError("HipRecurrentPPO: the policy's memories differ from the learner's")
        std = policy.std.detach()
        keep.append(std)
        return (lstm(ra), lstm(rc), arr(m.weight for m in la), arr(m.bias for m in la), arr(m.weight for m in lc), arr(m.bias for m in lc),
                C.c_void_p(std.data_ptr())), keep

    def load_from(self, policy):
        """The module's parameters become the learner's master parameters (device to device).  Adam's moments and step are kept."""
        if self.handle is None:
            self.policy = policy
            return
        args, _keep = self._arrays(policy)
        self._check(self.lib.rl_bptt_set_parameters(self.handle, *args, self._stream()))

    def store_into(self, policy):
        """The master parameters back into an ActorCriticRecurrent (for `state_dict()`: rsl_rl's checkpoint layout)."""
        if self.handle is None:
            if policy is not self.policy:
                policy.load_state_dict(self.policy.state_dict())
            return policy
        args, _keep = self._arrays(policy)
        self._check(self.lib.rl_bptt_get_parameters(self.handle, *args, self._stream()))
        return policy

    def sync_policy(self):
        """`store_into(self.policy)`: the module a checkpoint stores holds the learner's parameters afterwards"""
        return self.store_into(self.policy)

    def push(self, cell_a, cell_c, actor, critic, std_tensor):
        """The master parameters into the collection's kernels - the two `LstmCell`s, the two `MlpPolicy` heads, the sampling kernel's std tensor - on
        the current stream, without the host: `rl_lstm_set_weights_device` / `rl_mlp_set_weights_device` read the flat parameter buffer in place."""
        if self.handle is None:
            raise RlBpttError("HipRecurrentPPO.push before the handle exists: nothing to push")
        n = self.n_layers
        la, lc = (C.c_void_p * 4)(), (C.c_void_p * 4)()
        aw, ab, cw, cb = ((C.c_void_p * n)() for _ in range(4))
        sd = C.c_void_p()
        self._check(self.lib.rl_bptt_parameter_pointers(self.handle, la, lc, aw, ab, cw, cb, C.byref(sd)))
        for cell, ptrs in ((cell_a, la), (cell_c, lc)):
            if cell.lib.rl_lstm_set_weights_device(cell.handle, *[C.c_void_p(int(x)) for x in ptrs], self._stream()) != 0:
                raise RlBpttError("rl_lstm_set_weights_device: " + (cell.lib.rl_lstm_last_error() or b"").decode())
        actor.set_weights_device([int(x) for x in aw], [int(x) for x in ab])
        critic.set_weights_device([int(x) for x in cw], [int(x) for x in cb])
        if std_tensor.dtype != self._torch.float32 or not std_tensor.is_contiguous() or std_tensor.numel() != self.actor_dims[-1]:
            raise ValueError("HipRecurrentPPO.push: std_tensor must be a contiguous float32 tensor with one entry per action")
        none = C.POINTER(C.c_void_p)()
        self._check(self.lib.rl_bptt_get_parameters(self.handle, none, none, none, none, none, none, C.c_void_p(std_tensor.data_ptr()), self._stream()))

    def flat(self, which="parameters"):
        """A copy of a flat device buffer (`ActorCriticRecurrent.parameters()` order): "parameters", "gradients", "exp_avg", "exp_avg_sq"."""
        if self.handle is None:
            raise RlBpttError("HipRecurrentPPO.flat before the handle exists (pass num_steps= and num_envs=, or run an update)")
        out = self._torch.empty(self.num_parameters, device=self.device, dtype=self._torch.float32)
        self._check(self.lib.rl_bptt_get_flat(self.handle, FLATS.index(which), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- optimiser state (checkpoints) -------------------------------------------------------------------------------------------
    def optimizer_state_dict(self):
        """The layout of `torch.optim.Adam(policy.parameters()).state_dict()`: per-parameter `step`, `exp_avg`, `exp_avg_sq` in
        `ActorCriticRecurrent.parameters()` order and `param_groups[0]["lr"]`.  One wait of the current stream."""
        shapes = self.shapes()
        if self.handle is None:  # no update yet: what was loaded, or an optimiser that has not stepped
            zeros = self._torch.zeros(sum(math.prod(shp) for shp in shapes))
            return self._opt_pending if self._opt_pending is not None else adam_state_dict(shapes, zeros, zeros, 0, self.learning_rate)
        lr, step = C.c_double(), C.c_int64()
        self._check(self.lib.rl_bptt_get_optimizer(self.handle, C.byref(lr), C.byref(step), self._stream()))
        return adam_state_dict(shapes, self.flat("exp_avg"), self.flat("exp_avg_sq"), step.value, lr.value)

    def load_optimizer_state_dict(self, d):
        """An Adam `state_dict()` of this layout - written by this learner or by `recurrent.RecurrentPPO`'s optimizer - becomes the moments, the step
        counter and the learning-rate word (stream-ordered).  A state without entries (an optimiser that never stepped) zeroes the moments."""
        torch = self._torch
        m1, m2, step, lr = adam_state_flat(d, self.shapes())
        self.learning_rate = lr
        if self.handle is None:
            self._opt_pending = d
            return
        for which, m in ((2, m1), (3, m2)):
            m = torch.zeros(self.num_parameters, device=self.device) if m is None else m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.numel() != self.num_parameters:
                raise ValueError(f"optimizer state: {m.numel()} moment entries, the learner has {self.num_parameters} parameters")
            self._check(self.lib.rl_bptt_set_flat(self.handle, which, C.c_void_p(m.data_ptr()), self._stream()))  # (on torch's current stream: a temporary `m` is safe)
        self._check(self.lib.rl_bptt_set_optimizer(self.handle, lr, step, self._stream()))

    # -- the update -----------------------------------------------------------------------------------------------------------------
    def blocks(self, num_envs):
        """[(first env, one past the last)] of the mini-batches, as `RecurrentPPO.blocks`"""
        n = num_envs // self.num_mini_batches
        if n < 1:
            raise ValueError(f"HipRecurrentPPO: {num_envs} envs do not fill {self.num_mini_batches} mini-batches of whole trajectories")
        return [(i * n, (i + 1) * n) for i in range(self.num_mini_batches)]

    def _batch(self, batch):
        torch = self._torch
        obs = batch.observations
        if obs.ndim != 3:
            raise ValueError(f"HipRecurrentPPO: observations {tuple(obs.shape)} are not [T, N, obs]")
        T, N = int(obs.shape[0]), int(obs.shape[1])
        self.blocks(N)
        keep = []

        def ptr(t, shape, what, dtype=torch.float32):
            if t.dtype == torch.bool and dtype == torch.uint8:
                t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                t = t.to(device=self.device, dtype=dtype).contiguous()
            if t.numel() != math.prod(shape):
                raise ValueError(f"HipRecurrentPPO: {what} holds {tuple(t.shape)}, expected {shape}")
            keep.append(t)
            return t.data_ptr()

        A, H = self.actor_dims[-1], self.hidden
        (ha, ca), (hc, cc) = batch.hidden_a, batch.hidden_c
        b = BpttBatch(observations=ptr(obs, (T, N, self.obs_dim), "observations"),
                      privileged_observations=ptr(batch.privileged_observations, (T, N, self.critic_obs_dim), "privileged_observations"),
                      actions=ptr(batch.actions, (T, N, A), "actions"), values=ptr(batch.values, (T, N), "values"), returns=ptr(batch.returns, (T, N), "returns"),
                      advantages=ptr(batch.advantages, (T, N), "advantages"), actions_log_prob=ptr(batch.actions_log_prob, (T, N), "actions_log_prob"),
                      mu=ptr(batch.mu, (T, N, A), "mu"), sigma=ptr(batch.sigma, (T, N, A), "sigma"), dones=ptr(batch.dones, (T, N), "dones", torch.uint8),
                      h0_a=ptr(ha, (N, H), "hidden_a[0]"), c0_a=ptr(ca, (N, H), "hidden_a[1]"), h0_c=ptr(hc, (N, H), "hidden_c[0]"), c0_c=ptr(cc, (N, H), "hidden_c[1]"))
        self._need(T, N)
        return b, keep, T, N

    def _lo(self, lo, N):
        n = N // self.num_mini_batches
        if lo < 0 or lo + n > N:
            raise ValueError(f"HipRecurrentPPO: the block of {n} envs from {lo} leaves the {N} envs")
        return int(lo), n

    def block_grad(self, batch, lo):
        """Recurrence, heads, loss head and back-propagation through time for the block of envs lo .. lo + N // num_mini_batches - 1; returns the flat
        gradient.  No optimiser step, no statistics."""
        b, keep, T, N = self._batch(batch)
        lo, _n = self._lo(lo, N)
        self._check(self.lib.rl_bptt_block_grad(self.handle, C.byref(b), lo, self._stream()))
        return self.flat("gradients")

    def forward(self, batch, lo):
        """(mean [T, n, A], value [T, n]) of the same block: `ActorCriticRecurrent.unroll` on the learner's master parameters"""
        torch = self._torch
        b, keep, T, N = self._batch(batch)
        lo, n = self._lo(lo, N)
        mean = torch.empty(T, n, self.actor_dims[-1], device=self.device, dtype=torch.float32)
        value = torch.empty(T, n, device=self.device, dtype=torch.float32)
        self._check(self.lib.rl_bptt_forward(self.handle, C.byref(b), lo, C.c_void_p(mean.data_ptr()), C.c_void_p(value.data_ptr()), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # (keeps `keep` alive until the launches have read it)
        return mean, value

    def update(self, batch, generator=None) -> dict:
        """`RecurrentPPO.update`.  `generator` is not drawn from: there is no shuffle."""
        b, keep, T, N = self._batch(batch)
        self._check(self.lib.rl_bptt_update(self.handle, C.byref(b), self._stream()))
        out = (C.c_double * 8)()
        self._check(self.lib.rl_bptt_stats(self.handle, out, self._stream()))  # the one wait of the update (keeps `keep` alive until then)
        self.learning_rate, self.last_grad_norm, self.adam_step = float(out[4]), float(out[5]), int(out[7])
        return dict(value_loss=float(out[0]), surrogate_loss=float(out[1]), entropy=float(out[2]), kl=float(out[3]), learning_rate=self.learning_rate)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_bptt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        return (f"HipRecurrentPPO(obs={self.obs_dim}/{self.critic_obs_dim}, lstm={self.hidden}, actor={self.actor_dims}, critic={self.critic_dims}, "
                f"schedule={self.schedule!r}, lr={self.learning_rate:g}, librl_ppo_hip)")
