"""The LSTM cell of a recurrent policy's collection step on MI355X (`include/rl_lstm.h`, `csrc/rl_lstm.hip`).

What the reference's recurrent agent cfgs (`rsl_rl_recurrent_cfg_entry_point`: `RslRlRNNModelCfg(rnn_type="lstm", rnn_hidden_dim=256,
rnn_num_layers=1)`) run through rsl_rl's `Memory` in front of the actor's and the critic's MLP: one `nn.LSTM` step over all envs per
`alg.act(obs)`, and `Memory.reset(dones)` after `env.step`.  `LstmCell` is one cell (exact-f32 MFMA, gates in the launch's epilogue,
per-row reset and the state record folded in); `RecurrentState` is what a `robot_lab_amd.collect.Collector(recurrent=...)` carries from
step to step.  The rule the numbers follow is `robot_lab_amd/recurrent.py`.  There is no CPU fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LSTM_LIB = os.path.join(_HERE, "csrc", "librl_lstm_hip.so")
LSTM_EXPORTS = ["rl_lstm_create", "rl_lstm_set_weights_device", "rl_lstm_step", "rl_lstm_step_pair", "rl_lstm_in_dim", "rl_lstm_hidden", "rl_lstm_destroy",
                "rl_lstm_last_error"]
MAX_WIDTH = 512  # = RL_LSTM_MAX_WIDTH (include/rl_lstm.h)
_lib = None


class RlLstmError(RuntimeError):
    pass


def load_lstm_library(path: str | None = None) -> C.CDLL:
    global _lib
    path = path or os.environ.get("RL_LSTM_LIB") or LSTM_LIB  # RL_LSTM_LIB: alternative build (kernel analysis)
    if _lib is not None and path == LSTM_LIB:
        return _lib
    if not os.path.isfile(path):
        raise RlLstmError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback)")
    lib = C.CDLL(path)
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    lib.rl_lstm_create.argtypes = [C.c_int32, C.c_int32, fp, fp, fp, fp, C.c_int32, C.POINTER(vp)]
    lib.rl_lstm_set_weights_device.argtypes = [vp] * 6
    lib.rl_lstm_step.argtypes = [vp] * 10 + [C.c_int32, vp]
    lib.rl_lstm_step_pair.argtypes = [vp] * 19 + [C.c_int32, vp]
    lib.rl_lstm_in_dim.argtypes = [vp]
    lib.rl_lstm_hidden.argtypes = [vp]
    lib.rl_lstm_destroy.argtypes = [vp]
    lib.rl_lstm_last_error.restype = C.c_char_p
    if path == LSTM_LIB:
        _lib = lib
    return lib


def check_lstm_shapes(w_ih, w_hh, b_ih, b_hh):
    """(in_dim, hidden) of nn.LSTM's four single-layer tensors, or a ValueError that says what does not chain (no device needed)"""
    if len(w_hh.shape) != 2 or w_hh.shape[0] != 4 * w_hh.shape[1]:
        raise ValueError(f"LstmCell: weight_hh {tuple(w_hh.shape)} is not [4 hidden][hidden]")
    H = int(w_hh.shape[1])
    if len(w_ih.shape) != 2 or w_ih.shape[0] != 4 * H:
        raise ValueError(f"LstmCell: weight_ih {tuple(w_ih.shape)} is not [4 hidden = {4 * H}][in_dim]")
    D = int(w_ih.shape[1])
    if tuple(b_ih.shape) != (4 * H,) or tuple(b_hh.shape) != (4 * H,):
        raise ValueError(f"LstmCell: biases {tuple(b_ih.shape)} / {tuple(b_hh.shape)} are not [4 hidden = {4 * H}]")
    if not (1 <= D <= MAX_WIDTH and 1 <= H <= MAX_WIDTH):
        raise ValueError(f"LstmCell: in_dim {D} / hidden {H} out of range (1..{MAX_WIDTH})")
    return D, H


class LstmCell:
    """One single-layer LSTM cell on the GPU.  `w_ih` [4H, D], `w_hh` [4H, H], `b_ih`, `b_hh` [4H]: nn.LSTM's layout, gates i, f, g, o."""

    def __init__(self, w_ih, w_hh, b_ih, b_hh, device: str = "cuda:0", lib_path: str | None = None):
        import torch

        self._torch = torch
        to_np = lambda t: np.ascontiguousarray((t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float32, copy=False))  # noqa: E731
        arrs = [to_np(t) for t in (w_ih, w_hh, b_ih, b_hh)]
        self.in_dim, self.hidden = check_lstm_shapes(*arrs)
        self.lib = load_lstm_library(lib_path)
        self.device = torch.device(device)
        fp = C.POINTER(C.c_float)
        self.handle = C.c_void_p()
        if self.lib.rl_lstm_create(self.in_dim, self.hidden, *[a.ctypes.data_as(fp) for a in arrs], self.device.index or 0, C.byref(self.handle)) != 0:
            raise RlLstmError(self._err())

    @classmethod
    def from_module(cls, rnn, **kw):
        """from a single-layer `torch.nn.LSTM`"""
        return cls(rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, **kw)

    def _err(self):
        return (self.lib.rl_lstm_last_error() or b"").decode()

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _f32(self, t, shape, what, optional=False):
        if t is None and optional:
            return None
        if t is None or t.dtype != self._torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or t.device != self.device:
            raise ValueError(f"LstmCell: {what} must be a contiguous float32 tensor {tuple(shape)} on {self.device}" +
                             ("" if t is None else f", got {t.dtype} {tuple(t.shape)} on {t.device}"))
        return C.c_void_p(t.data_ptr())

    def _reset(self, reset, n):
        if reset is None:
            return None
        if reset.dtype not in (self._torch.uint8, self._torch.bool) or not reset.is_contiguous() or reset.numel() != n or reset.device != self.device:
            raise ValueError(f"LstmCell: reset must be a contiguous uint8 or bool tensor of {n} entries on {self.device}")
        return C.c_void_p(reset.data_ptr())

    def set_weights_device(self, w_ih, w_hh, b_ih, b_hh):
        """New parameters in place from float32 DEVICE tensors (`rl_lstm_set_weights_device`): a kernel on the current stream, capturable;
        the images keep their addresses.  The caller keeps the tensors alive until the stream has passed it."""
        D, H = self.in_dim, self.hidden
        args = [self._f32(t.detach(), s, n) for t, s, n in ((w_ih, (4 * H, D), "weight_ih"), (w_hh, (4 * H, H), "weight_hh"), (b_ih, (4 * H,), "bias_ih"), (b_hh, (4 * H,), "bias_hh"))]
        if self.lib.rl_lstm_set_weights_device(self.handle, *args, self._stream()) != 0:
            raise RlLstmError(self._err())

    def load_module(self, rnn):
        """`set_weights_device` from a single-layer `torch.nn.LSTM` whose parameters live on this device"""
        self.set_weights_device(rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)

    @staticmethod
    def _refuse_alias(ins, outs):
        for i in ins:
            lo, hi = i.data_ptr(), i.data_ptr() + i.numel() * 4
            for o in outs:
                if o is not None and o.data_ptr() < hi and lo < o.data_ptr() + o.numel() * 4:
                    raise ValueError("LstmCell: an output aliases the input state h / c - a workgroup reads rows while another writes them; "
                                     "ping-pong two buffers (RecurrentState does)")

    def _args(self, x, h, c, h_out, c_out, h_saved, c_saved, gates_out):
        n, D, H = x.shape[0], self.in_dim, self.hidden
        a = [self._f32(x, (n, D), "x"), self._f32(h, (n, H), "h"), self._f32(c, (n, H), "c"), self._f32(h_saved, (n, H), "h_saved", True),
             self._f32(c_saved, (n, H), "c_saved", True), self._f32(h_out, (n, H), "h_out"), self._f32(c_out, (n, H), "c_out"),
             self._f32(gates_out, (n, 4 * H), "gates_out", True)]
        self._refuse_alias((h, c), (h_out, c_out, h_saved, c_saved))
        return a

    def step(self, x, h, c, h_out, c_out, reset=None, h_saved=None, c_saved=None, gates_out=None):
        """(h_out, c_out) = cell(x, (h~, c~)), (h~, c~) = 0 on the rows with `reset`; `h_saved` / `c_saved` receive (h~, c~), `gates_out` the
        pre-activations [n, 4H] (include/rl_lstm.h rl_lstm_step)."""
        a = self._args(x, h, c, h_out, c_out, h_saved, c_saved, gates_out)
        n = x.shape[0]
        if self.lib.rl_lstm_step(self.handle, a[0], self._reset(reset, n), *a[1:], n, self._stream()) != 0:
            raise RlLstmError(self._err())
        return h_out, c_out

    def step_pair(self, x, h, c, h_out, c_out, other: "LstmCell", other_x, other_h, other_c, other_h_out, other_c_out, reset=None,
                  h_saved=None, c_saved=None, gates_out=None, other_h_saved=None, other_c_saved=None, other_gates_out=None):
        """two cells over the same rows and one reset vector in ONE launch (`rl_lstm_step_pair`): bit-identical to two `step` calls"""
        n = x.shape[0]
        if other_x.shape[0] != n or other.device != self.device:
            raise ValueError("LstmCell.step_pair needs two batches of the same row count on the same device")
        a = self._args(x, h, c, h_out, c_out, h_saved, c_saved, gates_out)
        b = other._args(other_x, other_h, other_c, other_h_out, other_c_out, other_h_saved, other_c_saved, other_gates_out)
        if self.lib.rl_lstm_step_pair(self.handle, *a, other.handle, *b, self._reset(reset, n), n, self._stream()) != 0:
            raise RlLstmError(self._err())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_lstm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class RecurrentState:
    """What a recurrent `Collector` carries: the actor's and the critic's cell, the ping-pong (h, c) buffers of both, the saved
    `[T, N, H]` tensors `h_a`, `c_a`, `h_c`, `c_c` (slot t: the state step t STARTED from, after its reset - what the update later starts
    a trajectory from) and the reset vector, which carries the last step's dones into the first step of the next iteration."""

    def __init__(self, cell_a: LstmCell, cell_c: LstmCell, num_envs: int, num_transitions_per_env: int):
        import torch

        if cell_a.device != cell_c.device:
            raise ValueError("RecurrentState: the two cells live on different devices")
        self.cell_a, self.cell_c, self.device = cell_a, cell_c, cell_a.device
        self.num_envs, self.T = num_envs, num_transitions_per_env
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
        N, T, Ha, Hc = num_envs, num_transitions_per_env, cell_a.hidden, cell_c.hidden
        self._ha, self._ca = (z(N, Ha), z(N, Ha)), (z(N, Ha), z(N, Ha))
        self._hc, self._cc = (z(N, Hc), z(N, Hc)), (z(N, Hc), z(N, Hc))
        self._k = 0  # which of the two buffers holds the current state
        self.h_a, self.c_a, self.h_c, self.c_c = z(T, N, Ha), z(T, N, Ha), z(T, N, Hc), z(T, N, Hc)
        self.reset = torch.zeros(N, dtype=torch.uint8, device=self.device)
        self._scratch = (z(N, Hc), z(N, Hc))  # the bootstrap call's (h', c'): written, never committed

    def state(self):
        """((h_a, c_a), (h_c, c_c)) as the next step will read them (before its reset)"""
        k = self._k
        return (self._ha[k], self._ca[k]), (self._hc[k], self._cc[k])

    def zero_(self):
        for t in (*self._ha, *self._ca, *self._hc, *self._cc, self.reset):
            t.zero_()

    def step(self, t: int, obs, critic_obs, reset):
        """Step t of an iteration: ONE pair launch - resets applied, the states saved into slot t; returns (h_a', h_c'), the rows the two MLP
        heads read.  `reset`: the uint8 / bool vector of the rows whose previous step ended an episode."""
        k = self._k
        self.cell_a.step_pair(obs, self._ha[k], self._ca[k], self._ha[1 - k], self._ca[1 - k], self.cell_c, critic_obs, self._hc[k], self._cc[k],
                              self._hc[1 - k], self._cc[1 - k], reset=reset, h_saved=self.h_a[t], c_saved=self.c_a[t], other_h_saved=self.h_c[t],
                              other_c_saved=self.c_c[t])
        self._k = 1 - k
        return self._ha[1 - k], self._hc[1 - k]

    def bootstrap(self, critic_obs, reset):
        """The critic's memory output for V(obs_T): from the current critic state (reset where the last step ended an episode) into scratch;
        NOTHING is committed - each observation enters the critic's memory once (robot_lab_amd/recurrent.py)."""
        k = self._k
        self.cell_c.step(critic_obs, self._hc[k], self._cc[k], self._scratch[0], self._scratch[1], reset=reset)
        return self._scratch[0]

    def close(self):
        self.cell_a.close()
        self.cell_c.close()
