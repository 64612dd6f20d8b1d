"""The HIP-native distillation learner (`include/rl_distill.h`, `csrc/learner/rl_distill.inl` inside librl_ppo_hip.so): `Distillation.update` of
`robot_lab_amd/distill.py` without torch autograd.

`distill.Distillation` stays the DEFINITION of the rule; `HipDistillation` evaluates the same rule - per-step behaviour loss (MSE or Huber),
groups of `gradient_length` steps whose count runs across the epochs, gradient-norm clipping, Adam - on fp32 master parameters of the STUDENT
that live on the device, with the PPO learner's GEMM / reduce / Adam kernels and a behaviour-cloning head.  One `update()` enqueues every group on
the current stream and reads ONE small statistics block afterwards.

    alg = HipDistillation(policy, num_envs=N, ...)   # same keywords as distill.Distillation; copies the student's parameters to the device
    stats = alg.update(batch)                        # {"behavior": ...}; batch.observations [T, N, obs], batch.teacher_actions [T, N, act]
    alg.push(student_mlp)                            # the master parameters into the inference kernel, device to device, current stream
    alg.store_into(policy)                           # back into the StudentTeacher (checkpoints keep rsl_rl's state_dict layout)
    alg.optimizer_state_dict()                       # the layout of torch.optim.Adam(policy.parameters()).state_dict(), state for the student's tensors

There is no CPU path and no fall-back to the torch learner: a missing library or an unsupported network raises."""
from __future__ import annotations

import ctypes as C

from .capi import PPO_LIB, RlPpoError
from .distill import LOSS_TYPES, student_shapes
from .ppo_hip import MAX_LAYERS, MAX_WIDTH, _network, adam_state_dict, adam_state_flat

DISTILL_EXPORTS = ["rl_distill_create", "rl_distill_destroy", "rl_distill_last_error", "rl_distill_num_parameters", "rl_distill_set_parameters",
                   "rl_distill_get_parameters", "rl_distill_parameter_pointers", "rl_distill_get_flat", "rl_distill_set_flat", "rl_distill_get_optimizer",
                   "rl_distill_set_optimizer", "rl_distill_group_grad", "rl_distill_update", "rl_distill_stats"]
_lib = None


class RlDistillError(RlPpoError):
    pass


class DistillHyper(C.Structure):
    """include/rl_distill.h `rl_distill_hyper`"""
    _fields_ = [("learning_rate", C.c_double), ("max_grad_norm", C.c_float), ("num_learning_epochs", C.c_int32), ("gradient_length", C.c_int32),
                ("loss_type", C.c_int32)]


def load_distill_library(path: str | None = None) -> C.CDLL:
    """the learner library (the PPO learner's: the distillation learner shares its kernels) with the prototypes of include/rl_distill.h"""
    global _lib
    import os

    path = path or os.environ.get("RL_PPO_LIB") or PPO_LIB
    if _lib is not None and path == PPO_LIB:
        return _lib
    if not os.path.isfile(path):
        raise RlDistillError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (the HIP learner has no CPU fallback)")
    lib = C.CDLL(path)
    if not hasattr(lib, "rl_distill_create"):
        raise RlDistillError(f"{path} has no rl_distill_create: this learner library predates the distillation learner, rebuild it")
    vp, pp = C.c_void_p, C.POINTER(C.c_void_p)
    lib.rl_distill_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(DistillHyper), C.c_int32, C.c_int32, pp]
    lib.rl_distill_destroy.argtypes = [vp]
    lib.rl_distill_last_error.restype = C.c_char_p
    lib.rl_distill_num_parameters.argtypes = [vp]
    lib.rl_distill_num_parameters.restype = C.c_int64
    lib.rl_distill_set_parameters.argtypes = [vp, pp, pp, vp]
    lib.rl_distill_get_parameters.argtypes = [vp, pp, pp, vp]
    lib.rl_distill_parameter_pointers.argtypes = [vp, pp, pp]
    lib.rl_distill_get_flat.argtypes = [vp, C.c_int32, vp, vp]
    lib.rl_distill_set_flat.argtypes = [vp, C.c_int32, vp, vp]
    lib.rl_distill_get_optimizer.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), vp]
    lib.rl_distill_set_optimizer.argtypes = [vp, C.c_double, C.c_int64, vp]
    lib.rl_distill_group_grad.argtypes = [vp, vp, vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp]
    lib.rl_distill_update.argtypes = [vp, vp, vp, C.c_int32, C.c_int32, vp]
    lib.rl_distill_stats.argtypes = [vp, C.POINTER(C.c_double), vp]
    if path == PPO_LIB:
        _lib = lib
    return lib


class HipDistillation:
    """`distill.Distillation` on the HIP learner: same constructor keywords plus `num_envs` (the N of every batch), same `update(batch) -> dict`."""

    def __init__(self, policy, num_envs, num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse",
                 lib_path: str | None = None):
        import torch

        self._torch = torch
        self.handle = None
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"HipDistillation: unknown loss_type {loss_type!r} (\"mse\" or \"huber\")")
        dims, act = _network(policy.student, "student")
        if act != "ELU":
            raise ValueError(f"HipDistillation: unsupported activation {act}: the HIP learner implements ELU only (use the torch learner, distill.Distillation)")
        if len(dims) - 1 > MAX_LAYERS or max(dims) > MAX_WIDTH:
            raise ValueError(f"HipDistillation: unsupported network: at most {MAX_LAYERS} layers of width <= {MAX_WIDTH} (got student {dims}); use the torch learner")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"HipDistillation: max_grad_norm={max_grad_norm!r} must be > 0, or None for no clipping")
        first = next(policy.student.parameters())
        if first.device.type != "cuda" or any(p.device != first.device for p in policy.parameters()):
            raise ValueError(f"HipDistillation: the policy must live on one CUDA device (the student is on {first.device}): the HIP learner has no CPU path - "
                             "move it with policy.to(\"cuda:0\") or use the torch learner, distill.Distillation")
        self.lib = load_distill_library(lib_path)
        self.policy, self.device = policy, first.device
        self.dims, self.n_layers, self.num_envs = dims, len(dims) - 1, int(num_envs)
        self.num_learning_epochs, self.gradient_length, self.learning_rate = int(num_learning_epochs), int(gradient_length), float(learning_rate)
        self.max_grad_norm, self.loss_type = max_grad_norm, loss_type
        self.last_grad_norm, self.num_updates = float("nan"), 0
        hp = DistillHyper(learning_rate=self.learning_rate, max_grad_norm=float(max_grad_norm or 0.0), num_learning_epochs=self.num_learning_epochs,
                          gradient_length=self.gradient_length, loss_type=LOSS_TYPES.index(loss_type))
        handle = C.c_void_p()
        rc = self.lib.rl_distill_create((C.c_int32 * len(dims))(*dims), self.n_layers, 0, C.byref(hp), self.num_envs, self.device.index or 0, C.byref(handle))
        self._check(rc)
        self.handle = handle
        self.num_parameters = int(self.lib.rl_distill_num_parameters(self.handle))
        self.load_from(policy)

    def _check(self, rc):
        if rc != 0:
            raise RlDistillError((self.lib.rl_distill_last_error() or b"").decode())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _arrays(self, policy):
        lin = [m for m in policy.student if isinstance(m, self._torch.nn.Linear)]
        if [lin[0].in_features] + [m.out_features for m in lin] != self.dims:
            raise ValueError("HipDistillation: the student's layer shapes differ from the learner's")
        keep = []

        def arr(params):
            out = []
            for t in params:
                t = t.detach()
                if t.dtype != self._torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"HipDistillation: parameters must be contiguous float32 tensors on {self.device}")
                keep.append(t)
                out.append(t.data_ptr())
            return (C.c_void_p * len(out))(*out)

        return arr(m.weight for m in lin), arr(m.bias for m in lin), keep

    def load_from(self, policy):
        """The student's parameters become the learner's master parameters (device to device).  Adam's moments and step are kept."""
        w, b, _keep = self._arrays(policy)
        self._check(self.lib.rl_distill_set_parameters(self.handle, w, b, self._stream()))

    def store_into(self, policy):
        """The master parameters back into a StudentTeacher's student (for `state_dict()`: rsl_rl's checkpoint layout)."""
        w, b, _keep = self._arrays(policy)
        self._check(self.lib.rl_distill_get_parameters(self.handle, w, b, self._stream()))
        return policy

    def push(self, student_mlp):
        """The master parameters into the inference kernel's image (`MlpPolicy`), on the current stream, without the host:
        `rl_mlp_set_weights_device` reads the flat parameter buffer in place."""
        n = self.n_layers
        w, b = (C.c_void_p * n)(), (C.c_void_p * n)()
        self._check(self.lib.rl_distill_parameter_pointers(self.handle, w, b))
        student_mlp.set_weights_device([int(x) for x in w], [int(x) for x in b])

    def flat(self, which="parameters"):
        """A copy of a flat device buffer (`student.parameters()` order): "parameters", "gradients", "exp_avg", "exp_avg_sq"."""
        out = self._torch.empty(self.num_parameters, device=self.device, dtype=self._torch.float32)
        self._check(self.lib.rl_distill_get_flat(self.handle, ["parameters", "gradients", "exp_avg", "exp_avg_sq"].index(which), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- optimiser state (checkpoints) -------------------------------------------------------------------------------------------
    def _all_shapes(self):
        """shapes of `policy.parameters()` (student, teacher, std); the first 2 L are the student's, the only ones with optimiser state"""
        return [tuple(p.shape) for p in self.policy.parameters()]

    def _student_ids(self):
        """the positions of the student's tensors in `policy.parameters()` (a module's own parameters - `std` - come before its children's)"""
        mine = [id(p) for p in self.policy.student.parameters()]
        pos = {id(p): i for i, p in enumerate(self.policy.parameters())}
        return [pos[i] for i in mine]

    def optimizer_state_dict(self):
        """The layout of `torch.optim.Adam(policy.parameters()).state_dict()`: one group over every parameter of the StudentTeacher, state
        (`step`, `exp_avg`, `exp_avg_sq`) for the student's tensors only - what the torch learner's optimiser holds, since nothing else ever
        receives a gradient.  One wait of the current stream."""
        lr, step = C.c_double(), C.c_int64()
        self._check(self.lib.rl_distill_get_optimizer(self.handle, C.byref(lr), C.byref(step), self._stream()))
        d = adam_state_dict(student_shapes(self.dims), self.flat("exp_avg"), self.flat("exp_avg_sq"), step.value, lr.value)
        ids = self._student_ids()
        d["state"] = {ids[i]: v for i, v in d["state"].items()}
        d["param_groups"][0]["params"] = list(range(len(self._all_shapes())))
        return d

    def load_optimizer_state_dict(self, d):
        """An Adam `state_dict()` of this layout - written by this learner or by `distill.Distillation`'s optimiser - becomes the moments, the
        step counter and the learning-rate word (stream-ordered).  A state without entries zeroes the moments."""
        torch = self._torch
        shapes, n_student = self._all_shapes(), 2 * self.n_layers
        groups = d["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(shapes):
            raise ValueError(f"optimizer state: expected one param group of {len(shapes)} parameters, got {[len(g['params']) for g in groups]}")
        ids = [list(groups[0]["params"])[i] for i in self._student_ids()]
        extra = [k for k in d["state"] if k not in ids]
        if extra:
            raise ValueError(f"optimizer state: parameters {extra} carry optimiser state, but only the student's tensors are trained")
        sub = dict(state={i: d["state"][k] for i, k in enumerate(ids) if k in d["state"]}, param_groups=[dict(groups[0], params=list(range(n_student)))])
        if sub["state"] and len(sub["state"]) != n_student:
            raise ValueError("optimizer state: some of the student's tensors have optimiser state and some have none")
        m1, m2, step, lr = adam_state_flat(sub, student_shapes(self.dims))
        for which, m in ((2, m1), (3, m2)):
            m = torch.zeros(self.num_parameters, device=self.device) if m is None else m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.numel() != self.num_parameters:
                raise ValueError(f"optimizer state: {m.numel()} moment entries, the learner has {self.num_parameters} parameters")
            self._check(self.lib.rl_distill_set_flat(self.handle, which, C.c_void_p(m.data_ptr()), self._stream()))
        self._check(self.lib.rl_distill_set_optimizer(self.handle, lr, step, self._stream()))
        self.learning_rate = lr

    # -- the update -----------------------------------------------------------------------------------------------------------------
    def _tensors(self, batch):
        torch = self._torch
        obs, ta = batch.observations, batch.teacher_actions
        if obs.ndim != 3 or ta.ndim != 3 or obs.shape[:2] != ta.shape[:2] or obs.shape[2] != self.dims[0] or ta.shape[2] != self.dims[-1]:
            raise ValueError(f"HipDistillation: observations {tuple(obs.shape)} / teacher_actions {tuple(ta.shape)} are not [T, N, {self.dims[0]}] / [T, N, {self.dims[-1]}]")
        if obs.shape[1] < 1 or obs.shape[1] > self.num_envs:
            raise ValueError(f"HipDistillation: {obs.shape[1]} envs in the batch, the learner was created for {self.num_envs}")
        fix = lambda t: t if t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() else t.to(device=self.device, dtype=torch.float32).contiguous()  # noqa: E731
        return fix(obs), fix(ta)

    def group_grad(self, batch, steps):
        """Forward, head and backward for the time steps `steps` (at most gradient_length of them); returns the flat gradient.  No optimiser step."""
        obs, ta = self._tensors(batch)
        steps = [int(t) for t in steps]
        if not steps or min(steps) < 0 or max(steps) >= obs.shape[0]:
            raise ValueError("HipDistillation.group_grad: steps must be time steps of the batch")
        arr = (C.c_int32 * len(steps))(*steps)
        self._check(self.lib.rl_distill_group_grad(self.handle, C.c_void_p(obs.data_ptr()), C.c_void_p(ta.data_ptr()), obs.shape[1], arr, len(steps), self._stream()))
        return self.flat("gradients")

    def update(self, batch) -> dict:
        obs, ta = self._tensors(batch)
        self._check(self.lib.rl_distill_update(self.handle, C.c_void_p(obs.data_ptr()), C.c_void_p(ta.data_ptr()), obs.shape[0], obs.shape[1], self._stream()))
        out = (C.c_double * 5)()
        self._check(self.lib.rl_distill_stats(self.handle, out, self._stream()))  # the one wait of the update (keeps obs / ta alive until then)
        self.learning_rate, self.last_grad_norm, self.num_updates = float(out[1]), float(out[2]), int(out[3])
        self.adam_step = int(out[4])
        return {"behavior": float(out[0])}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_distill_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        return (f"HipDistillation(student={self.dims}, gradient_length={self.gradient_length}, epochs={self.num_learning_epochs}, loss={self.loss_type!r}, "
                f"lr={self.learning_rate:g}, librl_ppo_hip)")
