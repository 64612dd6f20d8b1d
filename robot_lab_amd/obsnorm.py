"""Empirical observation normalisation on MI355X (`include/rl_obsnorm.h`, `csrc/rl_obsnorm.hip`).

The device half of `robot_lab_amd.ppo.EmpiricalNormalization`, which stays the definition of the rule: the running statistics are
updated inside the captured collection loop and applied in front of both networks by hand-written HIP kernels on the current torch
stream.  `mean`, `var`, `std` and `count` are torch views of the handle's own buffers (no copy); `load_module` / `store_module`
mirror an `EmpiricalNormalization`'s four buffers into and out of them.  No CPU fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
OBSNORM_LIB = os.path.join(_HERE, "csrc", "librl_obsnorm_hip.so")
OBSNORM_EXPORTS = ["rl_obsnorm_create", "rl_obsnorm_destroy", "rl_obsnorm_update", "rl_obsnorm_apply", "rl_obsnorm_update_pair", "rl_obsnorm_apply_pair",
                   "rl_obsnorm_get_state", "rl_obsnorm_set_state", "rl_obsnorm_state_pointers", "rl_obsnorm_dim", "rl_obsnorm_launch_count",
                   "rl_obsnorm_last_error"]
MAX_DIM = 512  # RL_OBSNORM_MAX_DIM
_lib = None


class RlObsNormError(RuntimeError):
    pass


def load_obsnorm_library(path: str | None = None) -> C.CDLL:
    global _lib
    path = path or os.environ.get("RL_OBSNORM_LIB") or OBSNORM_LIB  # RL_OBSNORM_LIB: alternative build (kernel analysis)
    if _lib is not None and path == OBSNORM_LIB:
        return _lib
    if not os.path.isfile(path):
        raise RlObsNormError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.rl_obsnorm_create.argtypes = [i32, C.c_float, i32, i32, C.POINTER(vp)]
    lib.rl_obsnorm_destroy.argtypes = [vp]
    lib.rl_obsnorm_update.argtypes = [vp, vp, i32, vp]
    lib.rl_obsnorm_apply.argtypes = [vp, vp, vp, i64, vp]
    lib.rl_obsnorm_update_pair.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.rl_obsnorm_apply_pair.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp]
    lib.rl_obsnorm_get_state.argtypes = [vp, vp, vp, vp, C.POINTER(i64), vp]
    lib.rl_obsnorm_set_state.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.rl_obsnorm_state_pointers.argtypes = [vp] + [C.POINTER(vp)] * 4
    lib.rl_obsnorm_dim.argtypes = [vp]
    lib.rl_obsnorm_dim.restype = i32
    lib.rl_obsnorm_launch_count.restype = i64
    lib.rl_obsnorm_last_error.restype = C.c_char_p
    if path == OBSNORM_LIB:
        _lib = lib
    return lib


class _DevView:
    def __init__(self, ptr, shape, typestr, owner):
        self._owner = owner
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


class ObsNormalizer:
    """`ObsNormalizer(dim, eps=1e-2, max_rows=N)`: one observation group's running statistics on the device.  Tensors passed in must be
    contiguous fp32 `[n_rows, dim]` on `device`."""

    def __init__(self, dim: int, eps: float = 1e-2, max_rows: int = 4096, device: str = "cuda:0", lib_path: str | None = None):
        import torch

        self._torch = torch
        self.lib = load_obsnorm_library(lib_path)
        self.device = torch.device(device)
        self.dim, self.eps, self.max_rows = int(dim), float(eps), int(max_rows)
        self.handle = C.c_void_p()
        if self.lib.rl_obsnorm_create(self.dim, self.eps, self.max_rows, self.device.index or 0, C.byref(self.handle)) != 0:
            self.handle = None
            raise RlObsNormError(self._err())
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.lib.rl_obsnorm_state_pointers(self.handle, *[C.byref(p) for p in ptrs]))
        view = lambda p, shape, ts: torch.as_tensor(_DevView(p.value, shape, ts, self), device=self.device)  # noqa: E731
        self.mean, self.var, self.std = (view(p, (1, self.dim), "<f4") for p in ptrs[:3])  # rsl_rl's buffer shapes
        self.count = view(ptrs[3], (1,), "<i8")

    def _err(self):
        return (self.lib.rl_obsnorm_last_error() or b"").decode()

    def _check(self, rc):
        if rc != 0:
            raise RlObsNormError(self._err())

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, x, what="x"):
        if x.dtype != self._torch.float32 or not x.is_contiguous() or x.ndim != 2 or x.shape[1] != self.dim or x.device != self.device:
            raise RlObsNormError(f"{what}: expected a contiguous fp32 tensor [n_rows, {self.dim}] on {self.device}, got {x.dtype} {tuple(x.shape)} on {x.device}")
        return C.c_void_p(x.data_ptr()) if x.numel() else C.c_void_p(x.data_ptr() or 8)  # (an empty tensor has no address: any non-NULL one)

    def _out(self, x, out):
        if out is None:
            return self._torch.empty_like(x)
        if out.shape != x.shape:
            raise RlObsNormError(f"out: shape {tuple(out.shape)} != {tuple(x.shape)}")
        return out

    def update(self, x):
        """`EmpiricalNormalization.update(x)` in training mode: one launch; zero rows change nothing."""
        self._check(self.lib.rl_obsnorm_update(self.handle, self._rows(x), x.shape[0], self._stream()))

    def apply(self, x, out=None):
        """`EmpiricalNormalization.forward(x)` -> `out` (allocated unless given; may be `x`)"""
        out = self._out(x, out)
        self._check(self.lib.rl_obsnorm_apply(self.handle, self._rows(x), self._rows(out, "out"), x.shape[0], self._stream()))
        return out

    def update_pair(self, x, other: "ObsNormalizer", other_x):
        if x.shape[0] != other_x.shape[0]:
            raise RlObsNormError("update_pair needs two batches of the same row count")
        self._check(self.lib.rl_obsnorm_update_pair(self.handle, self._rows(x), other.handle, other._rows(other_x), x.shape[0], self._stream()))

    def apply_pair(self, x, other: "ObsNormalizer", other_x, out=None, other_out=None):
        if x.shape[0] != other_x.shape[0]:
            raise RlObsNormError("apply_pair needs two batches of the same row count")
        out, other_out = self._out(x, out), other._out(other_x, other_out)
        self._check(self.lib.rl_obsnorm_apply_pair(self.handle, self._rows(x), self._rows(out, "out"), other.handle, other._rows(other_x),
                                                   other._rows(other_out, "out"), x.shape[0], self._stream()))
        return out, other_out

    def device_pointers(self):
        """(address of mean, address of std, eps): what a kernel that normalises for itself reads (`rl_ppo_set_obs_normalization`).  The
        addresses are fixed for the life of the handle; whoever keeps them keeps a reference to this object."""
        return self.mean.data_ptr(), self.std.data_ptr(), self.eps

    # -- state --------------------------------------------------------------------------------------------------------------------
    def set_state(self, mean, var, std, count: int):
        """the three vectors (fp32 device tensors of dim entries, any shape) and the count, stream-ordered (`rl_obsnorm_set_state`)"""
        torch = self._torch
        ts = [t.detach().to(device=self.device, dtype=torch.float32).reshape(-1).contiguous() for t in (mean, var, std)]
        if any(t.numel() != self.dim for t in ts):
            raise RlObsNormError(f"set_state: the vectors must hold {self.dim} entries")
        self._check(self.lib.rl_obsnorm_set_state(self.handle, *[C.c_void_p(t.data_ptr()) for t in ts], int(count), self._stream()))

    def get_state(self):
        """(mean, var, std) as new [1, dim] device tensors and the count as an int; waits for the stream (`rl_obsnorm_get_state`)"""
        ts = [self._torch.empty(1, self.dim, device=self.device, dtype=self._torch.float32) for _ in range(3)]
        n = C.c_int64()
        self._check(self.lib.rl_obsnorm_get_state(self.handle, *[C.c_void_p(t.data_ptr()) for t in ts], C.byref(n), self._stream()))
        return ts[0], ts[1], ts[2], int(n.value)

    def load_module(self, module):
        """an `EmpiricalNormalization`'s buffers become the device state"""
        for name in ("_mean", "_var", "_std"):
            if tuple(getattr(module, name).shape) != (1, self.dim):
                raise RlObsNormError(f"load_module: {name} has shape {tuple(getattr(module, name).shape)}, the handle's is (1, {self.dim})")
        self.set_state(module._mean, module._var, module._std, int(module.count))

    def store_module(self, module):
        """the device state back into the module's buffers (checkpoints, exporters): stream-ordered copies, no wait"""
        with self._torch.no_grad():
            module._mean.copy_(self.mean)
            module._var.copy_(self.var)
            module._std.copy_(self.std)
            module.count.copy_(self.count[0])
        return module

    def close(self):
        if getattr(self, "handle", None):
            for name in ("mean", "var", "std", "count"):
                if hasattr(self, name):
                    delattr(self, name)
            self.lib.rl_obsnorm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
