"""The HIP-native recurrent distillation learner (`include/rl_distill_bptt.h`, `csrc/learner/rl_distill_bptt.inl` inside librl_ppo_hip.so):
`RecurrentDistillation.update` of `robot_lab_amd/distill_recurrent.py` - truncated back-propagation through time - without torch autograd.

`distill_recurrent.RecurrentDistillation` stays the DEFINITION of the rule; `HipRecurrentDistillation` evaluates the same rule - the recurrence
restarted from the saved state every epoch, the input state zeroed behind a done, groups of `gradient_length` steps whose count runs across the
epochs, the state carried between groups as a value, gradient-norm clipping, Adam - on fp32 master parameters of the STUDENT (its memory and its
MLP) that live on the device.  One `update()` enqueues every group on the current stream and reads ONE small statistics block afterwards.

    alg = HipRecurrentDistillation(policy, num_envs=N, ...)  # same keywords as RecurrentDistillation; copies the student's parameters to the device
    stats = alg.update(batch)                                # {"behavior": ...}; batch: observations, teacher_actions, dones, h0, c0
    alg.final_state                                          # (h, c) [N, H] behind step T - 1 of the last epoch
    alg.push(cell, student_mlp)                              # the master parameters into the collection's kernels, device to device
    alg.store_into(policy)                                   # back into the StudentTeacherRecurrent (rsl_rl's state_dict layout)
    alg.optimizer_state_dict()                               # the layout of torch.optim.Adam(policy.trained_parameters()).state_dict()

There is no CPU path and no fall-back to the torch learner: a missing library or an unsupported network raises."""
from __future__ import annotations

import ctypes as C
import math

from .capi import PPO_LIB, RlPpoError
from .distill import LOSS_TYPES
from .distill_hip import DistillHyper
from .distill_recurrent import LSTM_NAMES, trained_shapes
from .ppo_hip import MAX_LAYERS, MAX_WIDTH, _network, adam_state_dict, adam_state_flat

RDISTILL_EXPORTS = ["rl_rdistill_create", "rl_rdistill_destroy", "rl_rdistill_last_error", "rl_rdistill_num_parameters", "rl_rdistill_set_parameters",
                    "rl_rdistill_get_parameters", "rl_rdistill_parameter_pointers", "rl_rdistill_get_flat", "rl_rdistill_set_flat", "rl_rdistill_get_optimizer",
                    "rl_rdistill_set_optimizer", "rl_rdistill_group_grad", "rl_rdistill_forward", "rl_rdistill_update", "rl_rdistill_final_state",
                    "rl_rdistill_stats"]
FLATS = ["parameters", "gradients", "exp_avg", "exp_avg_sq"]
_lib = None


class RlRdistillError(RlPpoError):
    pass


def load_rdistill_library(path: str | None = None) -> C.CDLL:
    """the learner library (the PPO learner's: this learner shares its kernels) with the prototypes of include/rl_distill_bptt.h"""
    global _lib
    import os

    path = path or os.environ.get("RL_PPO_LIB") or PPO_LIB
    if _lib is not None and path == PPO_LIB:
        return _lib
    if not os.path.isfile(path):
        raise RlRdistillError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (the HIP learner has no CPU fallback)")
    lib = C.CDLL(path)
    if not hasattr(lib, "rl_rdistill_create"):
        raise RlRdistillError(f"{path} has no rl_rdistill_create: this learner library predates the recurrent distillation learner, rebuild it")
    vp, pp, i32 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int32
    lib.rl_rdistill_create.argtypes = [i32, i32, C.POINTER(i32), i32, i32, C.POINTER(DistillHyper), i32, i32, pp]
    lib.rl_rdistill_destroy.argtypes = [vp]
    lib.rl_rdistill_last_error.restype = C.c_char_p
    lib.rl_rdistill_num_parameters.argtypes = [vp]
    lib.rl_rdistill_num_parameters.restype = C.c_int64
    lib.rl_rdistill_set_parameters.argtypes = [vp, pp, pp, pp, vp]
    lib.rl_rdistill_get_parameters.argtypes = [vp, pp, pp, pp, vp]
    lib.rl_rdistill_parameter_pointers.argtypes = [vp, pp, pp, pp]
    lib.rl_rdistill_get_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_rdistill_set_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_rdistill_get_optimizer.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), vp]
    lib.rl_rdistill_set_optimizer.argtypes = [vp, C.c_double, C.c_int64, vp]
    lib.rl_rdistill_group_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32), i32, vp]
    lib.rl_rdistill_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32), i32, vp, vp]
    lib.rl_rdistill_update.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
    lib.rl_rdistill_final_state.argtypes = [vp, vp, vp, vp]
    lib.rl_rdistill_stats.argtypes = [vp, C.POINTER(C.c_double), vp]
    if path == PPO_LIB:
        _lib = lib
    return lib


class HipRecurrentDistillation:
    """`distill_recurrent.RecurrentDistillation` on the HIP learner: same constructor keywords plus `num_envs` (the N of every batch), same
    `update(batch) -> dict` and `final_state`."""

    def __init__(self, policy, num_envs, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 lib_path: str | None = None):
        import torch

        from .distill_recurrent import StudentTeacherRecurrent

        self._torch = torch
        self.handle = None
        if not isinstance(policy, StudentTeacherRecurrent):
            raise TypeError(f"HipRecurrentDistillation: policy must be a StudentTeacherRecurrent, not {type(policy).__name__}")
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"HipRecurrentDistillation: unknown loss_type {loss_type!r} (\"mse\" or \"huber\")")
        dims, act = _network(policy.student, "student")
        if act != "ELU":
            raise ValueError(f"HipRecurrentDistillation: unsupported activation {act}: the HIP learner implements ELU only (use the torch learner, "
                             "distill_recurrent.RecurrentDistillation)")
        rnn, H = policy.memory_s.rnn, int(policy.rnn_hidden_dim)
        if not isinstance(rnn, torch.nn.LSTM) or rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias or rnn.hidden_size != H or getattr(rnn, "proj_size", 0):
            raise NotImplementedError(f"HipRecurrentDistillation: memory_s is not a single-layer, one-directional nn.LSTM of hidden size {H} with biases: GRU and "
                                      "stacked layers are not implemented (use the torch learner)")
        if len(dims) - 1 > MAX_LAYERS or max([rnn.input_size, H] + dims) > MAX_WIDTH or dims[0] != H:
            raise ValueError(f"HipRecurrentDistillation: unsupported network: a head of at most {MAX_LAYERS} layers behind a hidden state of {H}, every width <= "
                             f"{MAX_WIDTH} (got obs {rnn.input_size}, student {dims}); use the torch learner")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"HipRecurrentDistillation: max_grad_norm={max_grad_norm!r} must be > 0, or None for no clipping")
        first = rnn.weight_ih_l0
        if first.device.type != "cuda" or any(p.device != first.device for p in policy.parameters()):
            raise ValueError(f"HipRecurrentDistillation: the policy must live on one CUDA device (the student's memory is on {first.device}): the HIP learner has "
                             "no CPU path - move it with policy.to(\"cuda:0\") or use the torch learner, distill_recurrent.RecurrentDistillation")
        self.lib = load_rdistill_library(lib_path)
        self.policy, self.device = policy, first.device
        self.obs_dim, self.hidden, self.dims, self.n_layers, self.num_envs = int(rnn.input_size), H, dims, len(dims) - 1, int(num_envs)
        self.num_learning_epochs, self.gradient_length, self.learning_rate = int(num_learning_epochs), int(gradient_length), float(learning_rate)
        self.max_grad_norm, self.loss_type = max_grad_norm, loss_type
        self.last_grad_norm, self.num_updates = float("nan"), 0
        hp = DistillHyper(learning_rate=self.learning_rate, max_grad_norm=float(max_grad_norm or 0.0), num_learning_epochs=self.num_learning_epochs,
                          gradient_length=self.gradient_length, loss_type=LOSS_TYPES.index(loss_type))
        handle = C.c_void_p()
        rc = self.lib.rl_rdistill_create(self.obs_dim, H, (C.c_int32 * len(dims))(*dims), self.n_layers, 0, C.byref(hp), self.num_envs, self.device.index or 0,
                                         C.byref(handle))
        self._check(rc)
        self.handle = handle
        self.num_parameters = int(self.lib.rl_rdistill_num_parameters(self.handle))
        self._last_n = None
        self.load_from(policy)

    def _check(self, rc):
        if rc != 0:
            raise RlRdistillError((self.lib.rl_rdistill_last_error() or b"").decode())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def shapes(self):
        return trained_shapes(self.obs_dim, self.hidden, self.dims)

    def _arrays(self, policy):
        lin = [m for m in policy.student if isinstance(m, self._torch.nn.Linear)]
        rnn = policy.memory_s.rnn
        if [lin[0].in_features] + [m.out_features for m in lin] != self.dims or tuple(rnn.weight_ih_l0.shape) != (4 * self.hidden, self.obs_dim):
            raise ValueError("HipRecurrentDistillation: the student's shapes differ from the learner's")
        keep = []

        def arr(params):
            out = []
            for t in params:
                t = t.detach()
                if t.dtype != self._torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"HipRecurrentDistillation: parameters must be contiguous float32 tensors on {self.device}")
                keep.append(t)
                out.append(t.data_ptr())
            return (C.c_void_p * len(out))(*out)

        return arr(getattr(rnn, k) for k in LSTM_NAMES), arr(m.weight for m in lin), arr(m.bias for m in lin), keep

    def load_from(self, policy):
        """The student's parameters become the learner's master parameters (device to device).  Adam's moments and step are kept."""
        lstm, w, b, _keep = self._arrays(policy)
        self._check(self.lib.rl_rdistill_set_parameters(self.handle, lstm, w, b, self._stream()))

    def store_into(self, policy):
        """The master parameters back into a StudentTeacherRecurrent's student (for `state_dict()`: rsl_rl's checkpoint layout)."""
        lstm, w, b, _keep = self._arrays(policy)
        self._check(self.lib.rl_rdistill_get_parameters(self.handle, lstm, w, b, self._stream()))
        return policy

    def push(self, cell, student_mlp):
        """The master parameters into the collection's kernels - the student's `LstmCell` and its `MlpPolicy` head - on the current stream, without
        the host: `rl_lstm_set_weights_device` / `rl_mlp_set_weights_device` read the flat parameter buffer in place."""
        n = self.n_layers
        lstm, w, b = (C.c_void_p * 4)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        self._check(self.lib.rl_rdistill_parameter_pointers(self.handle, lstm, w, b))
        if cell.lib.rl_lstm_set_weights_device(cell.handle, *[C.c_void_p(int(x)) for x in lstm], self._stream()) != 0:
            raise RlRdistillError("rl_lstm_set_weights_device: " + (cell.lib.rl_lstm_last_error() or b"").decode())
        student_mlp.set_weights_device([int(x) for x in w], [int(x) for x in b])

    def flat(self, which="parameters"):
        """A copy of a flat device buffer (`trained_parameters()` order): "parameters", "gradients", "exp_avg", "exp_avg_sq"."""
        out = self._torch.empty(self.num_parameters, device=self.device, dtype=self._torch.float32)
        self._check(self.lib.rl_rdistill_get_flat(self.handle, FLATS.index(which), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- optimiser state (checkpoints) -------------------------------------------------------------------------------------------
    def optimizer_state_dict(self):
        """The layout of `torch.optim.Adam(policy.trained_parameters()).state_dict()` - what the torch learner's optimiser holds: per-parameter
        `step`, `exp_avg`, `exp_avg_sq` in `trained_parameters()` order and `param_groups[0]["lr"]`.  One wait of the current stream."""
        lr, step = C.c_double(), C.c_int64()
        self._check(self.lib.rl_rdistill_get_optimizer(self.handle, C.byref(lr), C.byref(step), self._stream()))
        return adam_state_dict(self.shapes(), self.flat("exp_avg"), self.flat("exp_avg_sq"), step.value, lr.value)

    def load_optimizer_state_dict(self, d):
        """An Adam `state_dict()` of this layout - written by this learner or by `RecurrentDistillation`'s optimiser - becomes the moments, the step
        counter and the learning-rate word (stream-ordered).  A state without entries zeroes the moments."""
        torch = self._torch
        m1, m2, step, lr = adam_state_flat(d, self.shapes())
        for which, m in ((2, m1), (3, m2)):
            m = torch.zeros(self.num_parameters, device=self.device) if m is None else m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.numel() != self.num_parameters:
                raise ValueError(f"optimizer state: {m.numel()} moment entries, the learner has {self.num_parameters} parameters")
            self._check(self.lib.rl_rdistill_set_flat(self.handle, which, C.c_void_p(m.data_ptr()), self._stream()))
        self._check(self.lib.rl_rdistill_set_optimizer(self.handle, lr, step, self._stream()))
        self.learning_rate = lr

    # -- the update -----------------------------------------------------------------------------------------------------------------
    def _tensors(self, batch, need_actions=True):
        torch = self._torch
        obs = batch.observations
        if obs.ndim != 3 or obs.shape[2] != self.obs_dim:
            raise ValueError(f"HipRecurrentDistillation: observations {tuple(obs.shape)} are not [T, N, {self.obs_dim}]")
        T, N = int(obs.shape[0]), int(obs.shape[1])
        if N < 1 or N > self.num_envs:
            raise ValueError(f"HipRecurrentDistillation: {N} envs in the batch, the learner was created for {self.num_envs}")
        keep = []

        def ptr(t, shape, what, dtype=torch.float32):
            if t.dtype == torch.bool and dtype == torch.uint8:
                t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                t = t.to(device=self.device, dtype=dtype).contiguous()
            if t.numel() != math.prod(shape):
                raise ValueError(f"HipRecurrentDistillation: {what} holds {tuple(t.shape)}, expected {shape}")
            keep.append(t)
            return C.c_void_p(t.data_ptr())

        A, H = self.dims[-1], self.hidden
        ta = ptr(batch.teacher_actions, (T, N, A), "teacher_actions") if need_actions else None
        return (ptr(obs, (T, N, self.obs_dim), "observations"), ta, ptr(batch.dones, (T, N), "dones", torch.uint8), ptr(batch.h0, (N, H), "h0"),
                ptr(batch.c0, (N, H), "c0")), keep, T, N

    def _group(self, steps, state, T, N, ptr_keep):
        steps = [int(t) for t in steps]
        if not steps or min(steps) < 0 or max(steps) >= T:
            raise ValueError("HipRecurrentDistillation: steps must be time steps of the batch")
        torch = self._torch
        h_in = c_in = None
        if state is not None:
            fix = lambda t: t if t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() else t.to(device=self.device, dtype=torch.float32).contiguous()  # noqa: E731
            hs, cs = fix(state[0]), fix(state[1])
            if tuple(hs.shape) != (N, self.hidden) or tuple(cs.shape) != (N, self.hidden):
                raise ValueError(f"HipRecurrentDistillation: the input state must be two [{N}, {self.hidden}] tensors")
            ptr_keep += [hs, cs]
            h_in, c_in = C.c_void_p(hs.data_ptr()), C.c_void_p(cs.data_ptr())
        return (C.c_int32 * len(steps))(*steps), len(steps), h_in, c_in

    def _final(self, N):
        torch = self._torch
        h, c = (torch.empty(N, self.hidden, device=self.device, dtype=torch.float32) for _ in range(2))
        self._check(self.lib.rl_rdistill_final_state(self.handle, C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), self._stream()))
        return h, c

    def group_grad(self, batch, steps, state=None):
        """Forward, head and back-propagation through time for the group of epoch-relative time steps `steps` in the rule's order (each the
        successor of the one before it, or 0), continuing from `state` = (h, c) before the first step's reset (not needed when steps[0] == 0).
        Returns (the flat gradient, the state behind the group's last step).  No optimiser step."""
        (obs, ta, dones, h0, c0), keep, T, N = self._tensors(batch)
        arr, n, h_in, c_in = self._group(steps, state, T, N, keep)
        self._check(self.lib.rl_rdistill_group_grad(self.handle, obs, ta, dones, h0, c0, h_in, c_in, N, arr, n, self._stream()))
        out = self.flat("gradients"), self._final(N)
        self._torch.cuda.current_stream(self.device).synchronize()  # (keeps `keep` alive until the launches have read it)
        return out

    def forward(self, batch, steps, state=None):
        """(mean [len(steps), N, A], the state behind the last step) of the same group on the learner's master parameters"""
        torch = self._torch
        (obs, _ta, dones, h0, c0), keep, T, N = self._tensors(batch, need_actions=False)
        arr, n, h_in, c_in = self._group(steps, state, T, N, keep)
        mean = torch.empty(n, N, self.dims[-1], device=self.device, dtype=torch.float32)
        self._check(self.lib.rl_rdistill_forward(self.handle, obs, dones, h0, c0, h_in, c_in, N, arr, n, C.c_void_p(mean.data_ptr()), self._stream()))
        out = mean, self._final(N)
        torch.cuda.current_stream(self.device).synchronize()
        return out

    def update(self, batch) -> dict:
        (obs, ta, dones, h0, c0), keep, T, N = self._tensors(batch)
        self._check(self.lib.rl_rdistill_update(self.handle, obs, ta, dones, h0, c0, T, N, self._stream()))
        self.final_state = self._final(N)
        out = (C.c_double * 5)()
        self._check(self.lib.rl_rdistill_stats(self.handle, out, self._stream()))  # the one wait of the update (keeps `keep` alive until then)
        self.learning_rate, self.last_grad_norm, self.num_updates = float(out[1]), float(out[2]), int(out[3])
        self.adam_step = int(out[4])
        return {"behavior": float(out[0])}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_rdistill_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        return (f"HipRecurrentDistillation(obs={self.obs_dim}, lstm={self.hidden}, student={self.dims}, gradient_length={self.gradient_length}, "
                f"epochs={self.num_learning_epochs}, loss={self.loss_type!r}, lr={self.learning_rate:g}, librl_ppo_hip)")
