"""ctypes binding of the C-ABI in ``include/rl_env.h``.

The product library is ``robot_lab_amd/csrc/librl_env_hip.so`` (hand-written HIP for gfx950, built by
``__graft_entry__.build()``).  There is no CPU fallback: if the library is missing or cannot be
loaded, :func:`load_library` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .desc import BUF, REAL_C, REAL_NP, EnvDesc, RL_LOG_SIZE

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(_HERE, "csrc", "librl_env_hip.so")

EXPORTS = [
    "rl_env_create", "rl_env_reset", "rl_env_step", "rl_env_step_record", "rl_env_get_buffer", "rl_env_export_state", "rl_env_commit_state",
    "rl_env_import_state", "rl_env_read_log", "rl_env_log_slot", "rl_env_obs_slot", "rl_env_step_count", "rl_env_set_step_count", "rl_env_num_envs", "rl_env_num_actions", "rl_env_obs_dim", "rl_env_max_episode_length", "rl_env_envs_per_wavefront", "rl_env_spec_id", "rl_env_plan",
    "rl_env_spec_source", "rl_env_register_spec_plugin", "rl_env_spec_plugin_count", "rl_env_abi_stamp",
    "rl_env_destroy", "rl_env_last_error", "rl_env_desc_size", "rl_env_graph_begin", "rl_env_graph_end", "rl_env_graph_launching",
    "rl_env_set_obs_history", "rl_env_obs_history",
]

_libs: dict[str, C.CDLL] = {}


class RlEnvError(RuntimeError):
    pass


def load_library(path: str | None = None) -> C.CDLL:
    path = path or os.environ.get("RL_ENV_LIB") or HIP_LIB  # RL_ENV_LIB: alternative HIP build (kernel ablations)
    if path in _libs:
        return _libs[path]
    if not os.path.isfile(path):
        raise RlEnvError(
            f"{path} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "robot_lab_amd has no CPU fallback.")
    lib = C.CDLL(path)
    fp = C.POINTER(REAL_C)
    lib.rl_env_create.argtypes = [C.POINTER(EnvDesc), fp, fp, fp, C.c_int32, C.c_uint64, C.c_int32, C.POINTER(C.c_void_p)]
    lib.rl_env_reset.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]
    lib.rl_env_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rl_env_step_record.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, REAL_C, C.c_void_p]
    lib.rl_env_get_buffer.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.rl_env_export_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.rl_env_commit_state.argtypes = [C.c_void_p, C.c_void_p]
    lib.rl_env_obs_slot.argtypes = [C.c_void_p]
    lib.rl_env_obs_slot.restype = C.c_int32
    lib.rl_env_step_count.argtypes = [C.c_void_p]
    lib.rl_env_step_count.restype = C.c_int64
    lib.rl_env_set_step_count.argtypes = [C.c_void_p, C.c_int64]
    lib.rl_env_import_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for n in ("rl_env_graph_begin", "rl_env_graph_end", "rl_env_graph_launching"):
        getattr(lib, n).argtypes = [C.c_void_p, C.c_void_p]
    lib.rl_env_read_log.argtypes = [C.c_void_p, fp, C.c_void_p]
    lib.rl_env_log_slot.argtypes = [C.c_void_p]
    lib.rl_env_log_slot.restype = C.c_int32
    for n in ("rl_env_num_envs", "rl_env_num_actions", "rl_env_max_episode_length", "rl_env_envs_per_wavefront", "rl_env_spec_id"):
        getattr(lib, n).argtypes = [C.c_void_p]
        getattr(lib, n).restype = C.c_int32
    lib.rl_env_plan.argtypes = [C.POINTER(EnvDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.rl_env_spec_source.argtypes = [C.POINTER(EnvDesc), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.rl_env_spec_source.restype = C.c_int
    lib.rl_env_register_spec_plugin.argtypes = [C.c_char_p]
    lib.rl_env_spec_plugin_count.restype = C.c_int32
    lib.rl_env_abi_stamp.restype = C.c_char_p
    lib.rl_env_obs_dim.argtypes = [C.c_void_p, C.c_int32]
    lib.rl_env_obs_dim.restype = C.c_int32
    if hasattr(lib, "rl_env_set_obs_history"):  # (absent from an RL_ENV_LIB build of an older tree - kernel A/Bs: such an env has no history, and asking for one raises)
        lib.rl_env_set_obs_history.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        lib.rl_env_obs_history.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        lib.rl_env_obs_history.restype = C.c_int32
    lib.rl_env_destroy.argtypes = [C.c_void_p]
    lib.rl_env_last_error.restype = C.c_char_p
    lib.rl_env_desc_size.restype = C.c_uint64
    if lib.rl_env_desc_size() != C.sizeof(EnvDesc):
        raise RlEnvError(f"ABI mismatch: library rl_env_desc is {lib.rl_env_desc_size()} bytes, Python mirror {C.sizeof(EnvDesc)}")
    _libs[path] = lib
    return lib


def _fptr(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=REAL_NP)
    return a, a.ctypes.data_as(C.POINTER(REAL_C))


def plan(desc: EnvDesc, num_envs: int, n_cu: int = 256, lib_path: str | None = None) -> dict:
    """`rl_env_plan`: the launch geometry `rl_env_create` would pick (no device needed)."""
    lib = load_library(lib_path)
    out = (C.c_int32 * 4)()
    if lib.rl_env_plan(C.byref(desc), num_envs, n_cu, out) != 0:
        raise RlEnvError((lib.rl_env_last_error() or b"").decode())
    return dict(lanes_per_limb=out[0], wavefronts_per_workgroup=out[1], lds_bytes_per_wavefront=out[2], lds_bytes_per_workgroup=out[3])


class NativeEnv:
    """Thin owner of an ``rl_env*``.  Pointers in/out are raw integers (device addresses for the HIP
    library, host addresses for the CPU lane emulator used by the tests)."""

    def __init__(self, desc: EnvDesc, heights, terrain_origins, env_origins, num_envs: int, seed: int, device: int = 0,
                 lib_path: str | None = None, obs_history: dict | None = None):
        self.lib = load_library(lib_path)
        self.handle = C.c_void_p()
        keep = []
        ptrs = []
        for a in (heights, terrain_origins, env_origins):
            r = _fptr(a)
            keep.append(r)
            ptrs.append(None if r is None else r[1])
        rc = self.lib.rl_env_create(C.byref(desc), ptrs[0], ptrs[1], ptrs[2], num_envs, C.c_uint64(seed & (2**64 - 1)), device, C.byref(self.handle))
        if rc != 0:
            raise RlEnvError(self.error())
        self.num_envs = num_envs
        self.num_actions = self.lib.rl_env_num_actions(self.handle)
        self.max_episode_length = self.lib.rl_env_max_episode_length(self.handle)
        # observation history (`rl_env_set_obs_history`): {"policy": [H_0, ...], "critic": [...]} per-term lengths, applied here - before
        # anybody fetches a buffer - and, because they are constructor arguments, again by whoever creates the env anew (the JIT path)
        for group, name in enumerate(("policy", "critic")):
            lengths = (obs_history or {}).get(name)
            if lengths is not None and any(int(h) != 0 for h in lengths):
                self.set_obs_history(group, lengths)

    def set_obs_history(self, group: int, lengths):
        if not hasattr(self.lib, "rl_env_set_obs_history"):
            raise RlEnvError("this env library predates observation history (rl_env_set_obs_history): rebuild it")
        arr = (C.c_int32 * len(lengths))(*[int(h) for h in lengths])
        self._check(self.lib.rl_env_set_obs_history(self.handle, group, arr, len(lengths)))

    def obs_history(self, group: int) -> list:
        if not hasattr(self.lib, "rl_env_obs_history"):
            return []
        out = (C.c_int32 * 64)()
        n = self.lib.rl_env_obs_history(self.handle, group, out, 64)
        if n < 0:
            raise RlEnvError("rl_env_obs_history failed")
        return [int(out[i]) for i in range(n)]

    def obs_dim(self, group: int) -> int:
        return int(self.lib.rl_env_obs_dim(self.handle, group))

    def envs_per_wavefront(self) -> int:
        return int(self.lib.rl_env_envs_per_wavefront(self.handle))

    def spec_id(self) -> int:
        """0: the term-stack interpreter; > 0: the step kernel specialised on this task (csrc/env_spec.h)."""
        return int(self.lib.rl_env_spec_id(self.handle))

    def error(self) -> str:
        return (self.lib.rl_env_last_error() or b"").decode()

    def _check(self, rc):
        if rc != 0:
            raise RlEnvError(self.error())

    def reset(self, env_ids=None, stream: int = 0):
        if env_ids is None:
            self._check(self.lib.rl_env_reset(self.handle, None, 0, C.c_void_p(stream)))
        else:
            ids = np.ascontiguousarray(env_ids, dtype=np.int32)
            self._check(self.lib.rl_env_reset(self.handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), C.c_void_p(stream)))

    def step(self, action_ptr: int, stream: int = 0):
        self._check(self.lib.rl_env_step(self.handle, C.c_void_p(action_ptr), C.c_void_p(stream)))

    def step_record(self, action_ptr: int, values_ptr: int, rewards_ptr: int, dones_ptr: int, gamma: float, stream: int = 0):
        self._check(self.lib.rl_env_step_record(self.handle, C.c_void_p(action_ptr), C.c_void_p(values_ptr), C.c_void_p(rewards_ptr),
                                                C.c_void_p(dones_ptr), gamma, C.c_void_p(stream)))

    def buffer(self, name: str):
        """-> (address, shape tuple, numpy dtype)"""
        ptr = C.c_void_p()
        shape = (C.c_int64 * 3)()
        nd, es = C.c_int32(), C.c_int32()
        self._check(self.lib.rl_env_get_buffer(self.handle, BUF[name], C.byref(ptr), shape, C.byref(nd), C.byref(es)))
        shp = tuple(int(shape[i]) for i in range(nd.value))
        dt = {"TERMINATED": np.uint8, "TIME_OUT": np.uint8, "EPISODE_LENGTH": np.int64, "TERRAIN_LEVEL": np.int32}.get(name, REAL_NP)
        if np.dtype(dt).itemsize != es.value:
            raise RlEnvError(f"buffer {name}: the library reports {es.value}-byte elements, the binding expects {np.dtype(dt)}")
        return ptr.value, shp, dt

    def export_state(self, stream: int = 0):
        self._check(self.lib.rl_env_export_state(self.handle, C.c_void_p(stream)))

    def commit_state(self, stream: int = 0):
        """AoS state buffers (ROOT_STATE, JOINT_*, ACTION, GAINS, CONTACT_TIMERS, TASK_STATE, ENV_ORIGIN) -> simulator state."""
        self._check(self.lib.rl_env_commit_state(self.handle, C.c_void_p(stream)))

    def obs_slot(self) -> int:
        return int(self.lib.rl_env_obs_slot(self.handle))

    @property
    def step_count(self) -> int:
        return int(self.lib.rl_env_step_count(self.handle))

    @step_count.setter
    def step_count(self, n: int):
        self._check(self.lib.rl_env_set_step_count(self.handle, int(n)))

    # hipGraph capture of a loop around step() (include/rl_env.h)
    def graph_begin(self, stream: int = 0):
        self._check(self.lib.rl_env_graph_begin(self.handle, C.c_void_p(stream)))

    def graph_end(self, stream: int = 0) -> int:
        n = self.lib.rl_env_graph_end(self.handle, C.c_void_p(stream))
        if n < 0:
            raise RlEnvError(self.error())
        return n

    def graph_launching(self, stream: int = 0):
        self._check(self.lib.rl_env_graph_launching(self.handle, C.c_void_p(stream)))

    def import_state(self, root_ptr=0, qpos_ptr=0, qvel_ptr=0, stream: int = 0):
        self._check(self.lib.rl_env_import_state(self.handle, C.c_void_p(root_ptr), C.c_void_p(qpos_ptr), C.c_void_p(qvel_ptr), C.c_void_p(stream)))

    def read_log(self, stream: int = 0) -> np.ndarray:
        out = np.zeros(RL_LOG_SIZE, dtype=REAL_NP)
        self._check(self.lib.rl_env_read_log(self.handle, out.ctypes.data_as(C.POINTER(REAL_C)), C.c_void_p(stream)))
        return out

    def log_slot(self) -> int:
        return int(self.lib.rl_env_log_slot(self.handle))

    def close(self):
        if self.handle:
            self.lib.rl_env_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- include/rl_ppo.h: the HIP PPO learner (csrc/rl_ppo.hip -> librl_ppo_hip.so; the host logic is robot_lab_amd/ppo_hip.py) ----------
PPO_LIB = os.path.join(_HERE, "csrc", "librl_ppo_hip.so")
PPO_EXPORTS = ["rl_ppo_create", "rl_ppo_destroy", "rl_ppo_last_error", "rl_ppo_num_parameters", "rl_ppo_set_parameters", "rl_ppo_get_parameters",
               "rl_ppo_parameter_pointers", "rl_ppo_get_flat", "rl_ppo_minibatch_grad", "rl_ppo_update", "rl_ppo_stats", "rl_ppo_set_symmetry",
               "rl_ppo_set_mirror_loss", "rl_ppo_stats_ex", "rl_ppo_set_world", "rl_ppo_wire", "rl_ppo_update_begin", "rl_ppo_minibatch_local",
               "rl_ppo_minibatch_apply", "rl_ppo_set_flat", "rl_ppo_get_optimizer", "rl_ppo_set_optimizer", "rl_ppo_set_obs_normalization"]
_ppo_lib = None


class RlPpoError(RuntimeError):
    pass


class Hyper(C.Structure):
    """include/rl_ppo.h `rl_ppo_hyper`"""
    _fields_ = [("learning_rate", C.c_double), ("desired_kl", C.c_double), ("value_loss_coef", C.c_float), ("clip_param", C.c_float),
                ("entropy_coef", C.c_float), ("max_grad_norm", C.c_float), ("use_clipped_value_loss", C.c_int32), ("num_learning_epochs", C.c_int32),
                ("num_mini_batches", C.c_int32), ("schedule", C.c_int32), ("std_type", C.c_int32)]


class Batch(C.Structure):
    """include/rl_ppo.h `rl_ppo_batch`"""
    _fields_ = [(n, C.c_void_p) for n in ("observations", "privileged_observations", "actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma")]


def load_ppo_library(path: str | None = None) -> C.CDLL:
    global _ppo_lib
    path = path or os.environ.get("RL_PPO_LIB") or PPO_LIB  # RL_PPO_LIB: alternative build (kernel ablations)
    if _ppo_lib is not None and path == PPO_LIB:
        return _ppo_lib
    if not os.path.isfile(path):
        raise RlPpoError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (the HIP learner has no CPU fallback)")
    lib = C.CDLL(path)
    pp = C.POINTER(C.c_void_p)
    lib.rl_ppo_create.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(Hyper), C.c_int32, C.c_int32, pp]
    lib.rl_ppo_destroy.argtypes = [C.c_void_p]
    lib.rl_ppo_last_error.restype = C.c_char_p
    lib.rl_ppo_num_parameters.argtypes = [C.c_void_p]
    lib.rl_ppo_num_parameters.restype = C.c_int64
    lib.rl_ppo_set_parameters.argtypes = [C.c_void_p, pp, pp, pp, pp, C.c_void_p, C.c_void_p]
    lib.rl_ppo_get_parameters.argtypes = [C.c_void_p, pp, pp, pp, pp, C.c_void_p, C.c_void_p]
    lib.rl_ppo_parameter_pointers.argtypes = [C.c_void_p, pp, pp, pp, pp, pp]
    lib.rl_ppo_get_flat.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rl_ppo_minibatch_grad.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p]
    lib.rl_ppo_update.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p]
    lib.rl_ppo_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.rl_ppo_set_symmetry.argtypes = [C.c_void_p, C.c_int32, ip, fp, ip, fp, ip, fp]
    lib.rl_ppo_set_mirror_loss.argtypes = [C.c_void_p, C.c_float, C.c_int32]
    lib.rl_ppo_stats_ex.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p]
    lib.rl_ppo_set_world.argtypes = [C.c_void_p, C.c_int32]
    lib.rl_ppo_wire.argtypes = [C.c_void_p, pp, C.POINTER(C.c_int64)]
    lib.rl_ppo_update_begin.argtypes = [C.c_void_p, C.c_void_p]
    lib.rl_ppo_minibatch_local.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_int32, C.c_void_p]
    lib.rl_ppo_minibatch_apply.argtypes = [C.c_void_p, C.c_void_p]
    lib.rl_ppo_set_flat.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rl_ppo_get_optimizer.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p]
    lib.rl_ppo_set_optimizer.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_void_p]
    lib.rl_ppo_set_obs_normalization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_float]
    if path == PPO_LIB:
        _ppo_lib = lib
    return lib
