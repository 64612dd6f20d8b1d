"""Random network distillation on MI355X: the device halves of `robot_lab_amd/rnd.py`, which stays the DEFINITION of the rule.

    reward = RndReward(num_envs, num_outputs, num_steps)          # include/rl_rnd.h (csrc/rl_rnd.hip, librl_rnd_hip.so): row norm, discounted average,
                                                                  # weight, the addition into the storage's reward slot, the sums for the log
    dev = RndDevice(rnd_module, num_envs, num_steps)              # the collection half: predictor + target as fused inference kernels (one pair launch),
    dev.begin_iteration(); dev.step(t, new_state, rewards[t])     # both normalisers as rl_obsnorm handles, the reward kernels; capturable
    alg = HipRND(rnd_module, num_learning_epochs, num_mini_batches, max_rows_per_minibatch, state_normalizer=dev.state_norm)
    alg.update(state_rows, perm)                                  # include/rl_rnd_learner.h (csrc/learner/rl_rnd.inl inside librl_ppo_hip.so): enqueues only
    alg.stats()                                                   # {"rnd_loss": ...}: the one wait
    alg.push(dev.predictor)                                       # the master parameters into the inference kernel, device to device

Either learner - `HipRND` here or the torch rule `rnd.update_minibatch` inside `ppo.PPO.update` - works on top of the same `RndDevice`.
There is no CPU path and no fall-back: a missing library or an unsupported network raises."""
from __future__ import annotations

import ctypes as C
import os

from .capi import PPO_LIB, RlPpoError
from .ppo_hip import MAX_LAYERS, MAX_WIDTH, _network, adam_state_dict, adam_state_flat

_HERE = os.path.dirname(os.path.abspath(__file__))
RND_LIB = os.path.join(_HERE, "csrc", "librl_rnd_hip.so")
RND_REWARD_EXPORTS = ["rl_rnd_reward_create", "rl_rnd_reward_destroy", "rl_rnd_reward_last_error", "rl_rnd_reward_set_weights", "rl_rnd_reward_rows",
                      "rl_rnd_reward_finish", "rl_rnd_reward_step", "rl_rnd_reward_pointers", "rl_rnd_reward_reset", "rl_rnd_reward_sums"]
RND_LEARNER_EXPORTS = ["rl_rnd_create", "rl_rnd_destroy", "rl_rnd_last_error", "rl_rnd_num_parameters", "rl_rnd_set_parameters", "rl_rnd_get_parameters",
                       "rl_rnd_parameter_pointers", "rl_rnd_get_flat", "rl_rnd_set_flat", "rl_rnd_get_optimizer", "rl_rnd_set_optimizer",
                       "rl_rnd_minibatch_grad", "rl_rnd_update", "rl_rnd_stats"]
MAX_OUTPUTS = 512  # RL_RND_MAX_OUTPUTS
_reward_lib = None
_learner_lib = None


class RlRndError(RuntimeError):
    pass


class RndHyper(C.Structure):
    """include/rl_rnd_learner.h `rl_rnd_hyper`"""
    _fields_ = [("learning_rate", C.c_double), ("num_learning_epochs", C.c_int32), ("num_mini_batches", C.c_int32)]


def load_rnd_reward_library(path: str | None = None) -> C.CDLL:
    global _reward_lib
    path = path or os.environ.get("RL_RND_LIB") or RND_LIB  # RL_RND_LIB: alternative build (kernel analysis)
    if _reward_lib is not None and path == RND_LIB:
        return _reward_lib
    if not os.path.isfile(path):
        raise RlRndError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32, fp = C.c_void_p, C.c_int32, C.POINTER(C.c_float)
    lib.rl_rnd_reward_create.argtypes = [i32, i32, i32, C.c_float, i32, C.POINTER(vp)]
    lib.rl_rnd_reward_destroy.argtypes = [vp]
    lib.rl_rnd_reward_last_error.restype = C.c_char_p
    lib.rl_rnd_reward_set_weights.argtypes = [vp, fp, vp]
    lib.rl_rnd_reward_rows.argtypes = [vp, vp, vp, vp]
    lib.rl_rnd_reward_finish.argtypes = [vp, i32, vp, vp, vp]
    lib.rl_rnd_reward_step.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.rl_rnd_reward_pointers.argtypes = [vp] + [C.POINTER(vp)] * 3
    lib.rl_rnd_reward_reset.argtypes = [vp, vp]
    lib.rl_rnd_reward_sums.argtypes = [vp, i32, C.POINTER(C.c_double), vp]
    if path == RND_LIB:
        _reward_lib = lib
    return lib


def load_rnd_learner_library(path: str | None = None) -> C.CDLL:
    """the learner library (the PPO learner's: the RND learner launches its kernels) with the prototypes of include/rl_rnd_learner.h"""
    global _learner_lib
    path = path or os.environ.get("RL_PPO_LIB") or PPO_LIB
    if _learner_lib is not None and path == PPO_LIB:
        return _learner_lib
    if not os.path.isfile(path):
        raise RlRndError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (the HIP learner has no CPU fallback)")
    lib = C.CDLL(path)
    if not hasattr(lib, "rl_rnd_create"):
        raise RlRndError(f"{path} has no rl_rnd_create: this learner library predates the RND learner, rebuild it")
    vp, pp, i32 = C.c_void_p, C.POINTER(C.c_void_p), C.c_int32
    lib.rl_rnd_create.argtypes = [C.POINTER(i32), i32, C.POINTER(i32), i32, i32, C.POINTER(RndHyper), i32, i32, pp]
    lib.rl_rnd_destroy.argtypes = [vp]
    lib.rl_rnd_last_error.restype = C.c_char_p
    lib.rl_rnd_num_parameters.argtypes = [vp]
    lib.rl_rnd_num_parameters.restype = C.c_int64
    lib.rl_rnd_set_parameters.argtypes = [vp, pp, pp, pp, pp, vp]
    lib.rl_rnd_get_parameters.argtypes = [vp, pp, pp, pp, pp, vp]
    lib.rl_rnd_parameter_pointers.argtypes = [vp, pp, pp]
    lib.rl_rnd_get_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_rnd_set_flat.argtypes = [vp, i32, vp, vp]
    lib.rl_rnd_get_optimizer.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), vp]
    lib.rl_rnd_set_optimizer.argtypes = [vp, C.c_double, C.c_int64, vp]
    lib.rl_rnd_minibatch_grad.argtypes = [vp, vp, vp, i32, vp]
    lib.rl_rnd_update.argtypes = [vp, vp, vp, i32, vp]
    lib.rl_rnd_stats.argtypes = [vp, C.POINTER(C.c_double), vp]
    if path == PPO_LIB:
        _learner_lib = lib
    return lib


class _DevView:
    def __init__(self, ptr, shape, typestr, owner):
        self._owner = owner
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


class RndReward:
    """include/rl_rnd.h: one handle per collector.  `r`, `avg`, `weights` are torch views of the handle's own buffers (no copy)."""

    def __init__(self, num_envs: int, num_outputs: int, num_steps: int, gamma: float = 0.99, device: str = "cuda:0", lib_path: str | None = None):
        import torch

        self._torch = torch
        self.lib = load_rnd_reward_library(lib_path)
        self.device = torch.device(device)
        self.num_envs, self.num_outputs, self.num_steps, self.gamma = int(num_envs), int(num_outputs), int(num_steps), float(gamma)
        self.handle = C.c_void_p()
        if self.lib.rl_rnd_reward_create(self.num_envs, self.num_outputs, self.num_steps, self.gamma, self.device.index or 0, C.byref(self.handle)) != 0:
            self.handle = None
            raise RlRndError(self._err())
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self.lib.rl_rnd_reward_pointers(self.handle, *[C.byref(p) for p in ptrs]))
        view = lambda p, n: torch.as_tensor(_DevView(p.value, (n,), "<f4", self), device=self.device)  # noqa: E731
        self.r, self.avg, self.weights = view(ptrs[0], self.num_envs), view(ptrs[1], self.num_envs), view(ptrs[2], self.num_steps)

    def _err(self):
        return (self.lib.rl_rnd_reward_last_error() or b"").decode()

    def _check(self, rc):
        if rc != 0:
            raise RlRndError(self._err())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _f32(self, t, shape, what):
        if t.dtype != self._torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or t.device != self.device:
            raise RlRndError(f"{what}: expected a contiguous fp32 tensor {tuple(shape)} on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return C.c_void_p(t.data_ptr())

    def set_weights(self, weights):
        """the [T] weights of the coming iteration (a sequence of floats): a stream-ordered copy, ahead of the loop or its graph launch"""
        if len(weights) != self.num_steps:
            raise RlRndError(f"set_weights: {len(weights)} weights, the handle has {self.num_steps} steps")
        self._check(self.lib.rl_rnd_reward_set_weights(self.handle, (C.c_float * self.num_steps)(*[float(w) for w in weights]), self._stream()))

    def rows(self, predictor, target):
        N, K = self.num_envs, self.num_outputs
        self._check(self.lib.rl_rnd_reward_rows(self.handle, self._f32(predictor, (N, K), "predictor"), self._f32(target, (N, K), "target"), self._stream()))

    def finish(self, t, reward_slot, std=None):
        """`std`: the [1, 1] std view of the reward's `ObsNormalizer` (dim 1), or None without reward normalisation"""
        sd = None if std is None else self._f32(std.view(-1), (1,), "std")
        self._check(self.lib.rl_rnd_reward_finish(self.handle, int(t), sd, self._f32(reward_slot, (self.num_envs,), "reward_slot"), self._stream()))

    def step(self, predictor, target, t, reward_slot):
        """rows + finish in ONE launch (no reward normalisation)"""
        N, K = self.num_envs, self.num_outputs
        self._check(self.lib.rl_rnd_reward_step(self.handle, self._f32(predictor, (N, K), "predictor"), self._f32(target, (N, K), "target"), int(t),
                                                self._f32(reward_slot, (N,), "reward_slot"), self._stream()))

    def reset(self):
        self._check(self.lib.rl_rnd_reward_reset(self.handle, self._stream()))

    def sums(self, n_steps=None):
        """(sum of the weighted intrinsic rewards, sum of the slot values after the addition) over the steps of the last loop; waits for the stream"""
        out = (C.c_double * 2)()
        self._check(self.lib.rl_rnd_reward_sums(self.handle, int(n_steps or self.num_steps), out, self._stream()))
        return float(out[0]), float(out[1])

    def close(self):
        if getattr(self, "handle", None):
            for name in ("r", "avg", "weights"):
                if hasattr(self, name):
                    delattr(self, name)
            self.lib.rl_rnd_reward_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class RndDevice:
    """The collection half of a `rnd.RandomNetworkDistillation` on the device: `step(t, new_state, reward_slot)` is `collect_step` of the rule as
    2 launches (the pair of networks, the reward kernel), + 2 with state normalisation (update, apply), + 2 with reward normalisation (the update
    of the dim-1 statistics with avg, the finish kernel).  The weights of an iteration are computed on the host from the module's schedule and the
    count of calls (`begin_iteration`) - the kernels of step t read entry t, so the loop can be captured once and replayed."""

    def __init__(self, module, num_envs: int, num_steps: int, device: str = "cuda:0"):
        import torch
        from torch import nn

        from .obsnorm import ObsNormalizer
        from .policy import MlpPolicy

        self._torch = torch
        self.module, self.num_envs, self.num_steps, self.device = module, int(num_envs), int(num_steps), torch.device(device)
        self.group = module.group
        pdims, pact = _network(module.predictor, "rnd predictor")
        tdims, tact = _network(module.target, "rnd target")
        if pact != "ELU" or tact != "ELU":
            raise ValueError(f"RndDevice: unsupported activation {pact} / {tact}: the fused inference kernels run ELU networks here")
        if max(pdims + tdims) > MAX_WIDTH or max(len(pdims), len(tdims)) - 1 > MAX_LAYERS:
            raise ValueError(f"RndDevice: unsupported network: at most {MAX_LAYERS} layers of width <= {MAX_WIDTH} (predictor {pdims}, target {tdims})")
        lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
        host = lambda t: t.detach().cpu().numpy()  # noqa: E731
        dev = str(self.device)
        self.predictor = MlpPolicy([host(x.weight) for x in lin(module.predictor)], [host(x.bias) for x in lin(module.predictor)], "elu", device=dev)
        self.target = MlpPolicy([host(x.weight) for x in lin(module.target)], [host(x.bias) for x in lin(module.target)], "elu", device=dev)
        self.state_norm = ObsNormalizer(module.state_dim, module.state_normalizer.eps, max_rows=self.num_envs, device=dev) if module.state_normalization else None
        self.reward_norm = ObsNormalizer(1, module.reward_normalizer.emp_norm.eps, max_rows=self.num_envs, device=dev) if module.reward_normalization else None
        gamma = module.reward_normalizer.gamma if module.reward_normalization else 0.99
        self.reward = RndReward(self.num_envs, module.num_outputs, self.num_steps, gamma, device=dev)
        self._scratch = torch.empty(self.num_envs, module.state_dim, device=self.device) if self.state_norm is not None else None
        self.last_weight = module.initial_weight

    def begin_iteration(self):
        """the weights of the next `num_steps` calls into the device vector (stream-ordered), the module's count of calls moved past them"""
        m = self.module
        w = [m.weight_at(m.update_counter + 1 + t) for t in range(self.num_steps)]
        m.update_counter += self.num_steps
        m.weight = self.last_weight = w[-1]
        self.reward.set_weights(w)

    def step(self, t, new_state, reward_slot):
        s = new_state
        if self.state_norm is not None:
            self.state_norm.update(new_state)
            s = self.state_norm.apply(new_state, out=self._scratch)
        p, g = self.predictor.forward_pair(s, self.target, s)
        if self.reward_norm is None:
            self.reward.step(p, g, t, reward_slot)
        else:
            self.reward.rows(p, g)
            self.reward_norm.update(self.reward.avg.view(-1, 1))
            self.reward.finish(t, reward_slot, self.reward_norm.std)

    def sync_module(self):
        """the normalisers' device state into the module's buffers (stream-ordered, no wait): what the torch learner, checkpoints and exporters read"""
        if self.state_norm is not None:
            self.state_norm.store_module(self.module.state_normalizer)
        if self.reward_norm is not None:
            self.reward_norm.store_module(self.module.reward_normalizer.emp_norm)

    def load_module(self, predictor=True):
        """after a `load_state_dict` of the module: both networks and the normalisers' buffers into the device images (`predictor=False`: a HIP
        learner holds the predictor's master parameters and pushes them itself)"""
        if predictor:
            self.predictor.load_linear_layers(self.module.predictor)
        self.target.load_linear_layers(self.module.target)
        if self.state_norm is not None:
            self.state_norm.load_module(self.module.state_normalizer)
        if self.reward_norm is not None:
            self.reward_norm.load_module(self.module.reward_normalizer.emp_norm)

    def close(self):
        for h in (self.predictor, self.target, self.state_norm, self.reward_norm, self.reward):
            if h is not None:
                h.close()


def predictor_shapes(dims):
    shapes = []
    for l in range(len(dims) - 1):
        shapes += [(dims[l + 1], dims[l]), (dims[l + 1],)]
    return shapes


class HipRND:
    """The update half on the HIP learner: the rule is `rnd.update_minibatch` per mini-batch of `PPO.update`.  `state_normalizer`: the `ObsNormalizer`
    handle of the collection (`RndDevice.state_norm`) when the module normalises its state - `update` then runs ONE `rl_obsnorm_apply` over the stored
    rows into a scratch matrix, with the statistics as the collection left them."""

    def __init__(self, module, num_learning_epochs=5, num_mini_batches=4, max_rows_per_minibatch=None, state_normalizer=None, lib_path: str | None = None):
        import torch

        self._torch = torch
        self.handle = None
        pdims, pact = _network(module.predictor, "rnd predictor")
        tdims, tact = _network(module.target, "rnd target")
        if pact != "ELU" or tact != "ELU":
            raise ValueError(f"HipRND: unsupported activation {pact} / {tact}: the HIP learner implements ELU only (use the torch learner, rnd.update_minibatch)")
        if max(len(pdims), len(tdims)) - 1 > MAX_LAYERS or max(pdims + tdims) > MAX_WIDTH:
            raise ValueError(f"HipRND: unsupported network: at most {MAX_LAYERS} layers of width <= {MAX_WIDTH} (got predictor {pdims}, target {tdims})")
        if bool(module.state_normalization) != (state_normalizer is not None):
            raise ValueError("HipRND: state_normalizer= must be the collection's ObsNormalizer handle exactly when the module has state_normalization")
        first = next(module.predictor.parameters())
        if first.device.type != "cuda" or any(p.device != first.device for p in module.parameters()):
            raise ValueError(f"HipRND: the module must live on one CUDA device (the predictor is on {first.device}): the HIP learner has no CPU path")
        if not max_rows_per_minibatch or int(max_rows_per_minibatch) < 1:
            raise ValueError("HipRND: max_rows_per_minibatch (the rows of the largest mini-batch) must be given")
        self.lib = load_rnd_learner_library(lib_path)
        self.module, self.device, self.group = module, first.device, module.group
        self.pdims, self.tdims = pdims, tdims
        self.num_learning_epochs, self.num_mini_batches, self.learning_rate = int(num_learning_epochs), int(num_mini_batches), float(module.learning_rate)
        self.max_rows, self.state_normalizer = int(max_rows_per_minibatch), state_normalizer
        self._scratch = None
        hp = RndHyper(learning_rate=self.learning_rate, num_learning_epochs=self.num_learning_epochs, num_mini_batches=self.num_mini_batches)
        handle = C.c_void_p()
        i32 = C.c_int32
        rc = self.lib.rl_rnd_create((i32 * len(pdims))(*pdims), len(pdims) - 1, (i32 * len(tdims))(*tdims), len(tdims) - 1, 0, C.byref(hp), self.max_rows,
                                    self.device.index or 0, C.byref(handle))
        self._check(rc)
        self.handle = handle
        self.num_parameters = int(self.lib.rl_rnd_num_parameters(self.handle))
        self.load_from(module)

    def _check(self, rc):
        if rc != 0:
            raise RlRndError((self.lib.rl_rnd_last_error() or b"").decode())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _arrays(self, module):
        nn = self._torch.nn
        lp, lt = [m for m in module.predictor if isinstance(m, nn.Linear)], [m for m in module.target if isinstance(m, nn.Linear)]
        if [lp[0].in_features] + [m.out_features for m in lp] != self.pdims or [lt[0].in_features] + [m.out_features for m in lt] != self.tdims:
            raise ValueError("HipRND: the module's layer shapes differ from the learner's")
        keep = []

        def arr(params):
            out = []
            for t in params:
                t = t.detach()
                if t.dtype != self._torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"HipRND: parameters must be contiguous float32 tensors on {self.device}")
                keep.append(t)
                out.append(t.data_ptr())
            return (C.c_void_p * len(out))(*out)

        return arr(m.weight for m in lp), arr(m.bias for m in lp), arr(m.weight for m in lt), arr(m.bias for m in lt), keep

    def load_from(self, module):
        """both networks' parameters become the learner's (device to device).  Adam's moments and step are kept."""
        pw, pb, tw, tb, _keep = self._arrays(module)
        self._check(self.lib.rl_rnd_set_parameters(self.handle, pw, pb, tw, tb, self._stream()))

    def store_into(self, module):
        """the predictor's master parameters back into the module (the target never changed)"""
        pw, pb, _tw, _tb, _keep = self._arrays(module)
        self._check(self.lib.rl_rnd_get_parameters(self.handle, pw, pb, None, None, self._stream()))
        return module

    def target_parameters(self):
        """copies of the target's tensors as the learner holds them (tests: the target is never written)"""
        torch = self._torch
        n = len(self.tdims) - 1
        ws = [torch.empty(self.tdims[l + 1], self.tdims[l], device=self.device) for l in range(n)]
        bs = [torch.empty(self.tdims[l + 1], device=self.device) for l in range(n)]
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        self._check(self.lib.rl_rnd_get_parameters(self.handle, None, None, arr(ws), arr(bs), self._stream()))
        return ws, bs

    def push(self, predictor_mlp):
        """the predictor's master parameters into the inference kernel's image (`MlpPolicy`), on the current stream, without the host"""
        n = len(self.pdims) - 1
        w, b = (C.c_void_p * n)(), (C.c_void_p * n)()
        self._check(self.lib.rl_rnd_parameter_pointers(self.handle, w, b))
        predictor_mlp.set_weights_device([int(x) for x in w], [int(x) for x in b])

    def flat(self, which="parameters"):
        """A copy of a flat device buffer (`predictor.parameters()` order): "parameters", "gradients", "exp_avg", "exp_avg_sq"."""
        out = self._torch.empty(self.num_parameters, device=self.device, dtype=self._torch.float32)
        self._check(self.lib.rl_rnd_get_flat(self.handle, ["parameters", "gradients", "exp_avg", "exp_avg_sq"].index(which), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- optimiser state (checkpoints): the layout of torch.optim.Adam(predictor.parameters()).state_dict() ---------------------------------
    def optimizer_state_dict(self):
        lr, step = C.c_double(), C.c_int64()
        self._check(self.lib.rl_rnd_get_optimizer(self.handle, C.byref(lr), C.byref(step), self._stream()))
        return adam_state_dict(predictor_shapes(self.pdims), self.flat("exp_avg"), self.flat("exp_avg_sq"), step.value, lr.value)

    def load_optimizer_state_dict(self, d):
        torch = self._torch
        m1, m2, step, lr = adam_state_flat(d, predictor_shapes(self.pdims))
        for which, m in ((2, m1), (3, m2)):
            m = torch.zeros(self.num_parameters, device=self.device) if m is None else m.to(device=self.device, dtype=torch.float32).contiguous()
            if m.numel() != self.num_parameters:
                raise ValueError(f"optimizer state: {m.numel()} moment entries, the learner has {self.num_parameters} parameters")
            self._check(self.lib.rl_rnd_set_flat(self.handle, which, C.c_void_p(m.data_ptr()), self._stream()))
        self._check(self.lib.rl_rnd_set_optimizer(self.handle, lr, step, self._stream()))
        self.learning_rate = lr

    # -- the update --------------------------------------------------------------------------------------------------------------------------
    def _state(self, state_rows):
        """the [rows, S] matrix the kernels gather from: the stored rows, through the state normaliser's scratch pass when there is one"""
        torch = self._torch
        t = state_rows
        if t.ndim != 2 or t.shape[1] != self.pdims[0]:
            raise ValueError(f"HipRND: state rows {tuple(t.shape)} are not [rows, {self.pdims[0]}]")
        if t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if self.state_normalizer is not None:
            if self._scratch is None or self._scratch.shape != t.shape:
                self._scratch = torch.empty_like(t)
            t = self.state_normalizer.apply(t, out=self._scratch)
        return t

    def _perm(self, perm, rows):
        perm = perm.to(device=self.device, dtype=self._torch.int64).contiguous()
        if perm.numel() < 1 or int(perm.min()) < 0 or int(perm.max()) >= rows:
            raise ValueError("HipRND: the row numbers must index the state rows")
        return perm

    def minibatch_grad(self, state_rows, idx):
        """forward, head and the predictor's backward on the rows `idx`; returns the flat gradient.  No optimiser step."""
        s = self._state(state_rows)
        idx = self._perm(idx, s.shape[0])
        self._check(self.lib.rl_rnd_minibatch_grad(self.handle, C.c_void_p(s.data_ptr()), C.c_void_p(idx.data_ptr()), idx.numel(), self._stream()))
        return self.flat("gradients")

    def update(self, state_rows, perm, checked=False):
        """enqueues epochs x mini-batches over `perm` (the permutation of the PPO update); `stats()` afterwards is the one wait"""
        s = self._state(state_rows)
        if not checked:
            perm = self._perm(perm, s.shape[0])
        self._keep = (s, perm)
        self._check(self.lib.rl_rnd_update(self.handle, C.c_void_p(s.data_ptr()), C.c_void_p(perm.data_ptr()), perm.numel(), self._stream()))

    def stats(self) -> dict:
        out = (C.c_double * 4)()
        self._check(self.lib.rl_rnd_stats(self.handle, out, self._stream()))
        self._keep = None
        self.learning_rate, self.adam_step = float(out[1]), int(out[3])
        return {"rnd_loss": float(out[0])}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_rnd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __repr__(self):
        return f"HipRND(predictor={self.pdims}, target={self.tdims}, lr={self.learning_rate:g}, librl_ppo_hip)"


__all__ = ["HipRND", "RndDevice", "RndReward", "RlRndError", "RlPpoError", "RND_REWARD_EXPORTS", "RND_LEARNER_EXPORTS"]
