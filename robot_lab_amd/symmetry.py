"""Symmetry data augmentation on MI355X (`include/rl_rollout.h`: `rl_symmetry_*`, `csrc/rl_rollout.hip`).

Host-side mirror of the reference's `compute_symmetric_states(env, obs, actions)`
(`source/robot_lab/robot_lab/tasks/manager_based/locomotion/velocity/mdp/symmetry/anymal.py:27-87`), the function an
rsl_rl PPO configured with `RslRlSymmetryCfg(use_data_augmentation=True, data_augmentation_func=...)` calls on every
mini-batch (`.../config/quadruped/anymal_d/agents/rsl_rl_ppo_cfg.py:100-105`).  Each of the four copies (identity,
left-right, front-back, diagonal) is a signed column permutation; the tables are built here from the joint names and the
observation layout, the copies are produced by one HIP kernel launch.  No CPU fallback.

The same tables drive the augmentation INSIDE the PPO update (`ppo.PPO(symmetry=...)`, `ppo_hip.HipPPO(symmetry=...)`,
`ppo.Trainer(env, symmetry="lr")`): `tables_for_env` builds them for the robots this project runs from the joint names and the
observation term lists of the env descriptor, `SymmetryTables` carries and checks them.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import re

import numpy as np

from .rollout import RlRolloutError, load_rollout_library

SYMMETRY_EXPORTS = ["rl_symmetry_create", "rl_symmetry_apply", "rl_symmetry_destroy"]
# ANYmal articulation order (anymal.py:216-229)
ANYMAL_JOINTS = ["LF_HAA", "LH_HAA", "RF_HAA", "RH_HAA", "LF_HFE", "LH_HFE", "RF_HFE", "RH_HFE", "LF_KFE", "LH_KFE", "RF_KFE", "RH_KFE"]
# what a mirror does to the components of a base-frame quantity: (left-right, front-back)
_VEC = dict(lin=((1, -1, 1), (-1, 1, 1)),       # polar vectors: linear velocity, projected gravity
            ang=((-1, 1, -1), (1, -1, -1)),     # axial vectors: angular velocity
            cmd=((1, -1, -1), (-1, 1, -1)))     # (v_x, v_y, omega_z) velocity command


# Unitree-style articulations (A1, Go2, B2 and the wheeled Go2W, B2W): <end><side>_<kind>_joint, the rear end labelled R, roll joint `hip`
UNITREE_PATTERN = r"(?P<end>[FR])(?P<side>[LR])_(?P<kind>hip|thigh|calf|foot)_joint"
UNITREE = dict(pattern=UNITREE_PATTERN, roll_kinds=("hip",), ends=("F", "R"))
MAX_SYM = 8  # = RL_PPO_MAX_SYM (include/rl_ppo.h)


def joint_tables(joint_names, pattern=r"(?P<side>[LR])(?P<end>[FH])_(?P<kind>\w+)", roll_kinds=("HAA",), ends=("F", "H")):
    """(perm, sign) of the left-right and the front-back mirror on a per-joint vector: out[j] = sign[j] * in[perm[j]].
    Left-right swaps the L and R legs and flips the roll (abduction) joints; front-back swaps the two `ends` (front, rear
    label) and flips the pitch joints (everything that is not a roll joint).

    The `foot` joints of the wheeled robots are "not roll", and that is right for a wheel: every wheel spins about +y of its calf
    on either side (the descriptors' link_axis), so its angle, velocity and velocity target are the y component of an AXIAL
    vector.  A mirror multiplies an axial component by -1 if it lies IN the mirror plane and by +1 if it is NORMAL to it
    (`_VEC["ang"]`): y is normal to the left-right plane (x-z) -> the wheels swap sides with sign +1 (both wheels of a robot
    driving forward spin the same way, before and after); y lies in the front-back plane (y-z) -> the wheels swap ends with
    sign -1 (the mirrored robot drives backward).  The thigh and calf joints, also about y, go the same way."""
    parsed = []
    for n in joint_names:
        m = re.fullmatch(pattern, n)
        if m is None:
            raise ValueError(f"joint name {n!r} does not match {pattern!r}")
        parsed.append((m["side"], m["end"], m["kind"]))
    index = {p: i for i, p in enumerate(parsed)}
    lr_p, lr_s, fb_p, fb_s = [], [], [], []
    for side, end, kind in parsed:
        lr_p.append(index[("R" if side == "L" else "L", end, kind)])
        lr_s.append(-1.0 if kind in roll_kinds else 1.0)
        fb_p.append(index[(side, ends[1] if end == ends[0] else ends[0], kind)])
        fb_s.append(1.0 if kind in roll_kinds else -1.0)
    return (np.array(lr_p), np.array(lr_s)), (np.array(fb_p), np.array(fb_s))


def layout_tables(layout, joint_names=ANYMAL_JOINTS, scan=None, **kw):
    """perm [4, dim] (int32) and sign [4, dim] (float32) of the copies (identity, left-right, front-back, diagonal =
    front-back of left-right) for a row made of `layout` blocks: "lin" | "ang" | "cmd" (3 columns), "joint" (one
    column per joint) or "scan" (the height scan, `scan` = (nx, ny) columns: a centred, yaw-aligned grid flattened
    iy * nx + ix; left-right maps iy -> ny - 1 - iy, front-back ix -> nx - 1 - ix, a height keeps its sign)."""
    (lrp, lrs), (fbp, fbs) = joint_tables(joint_names, **kw)
    perms, signs = [[], []], [[], []]
    off = 0
    if "scan" in layout:
        if scan is None or min(scan) < 1:
            raise ValueError("a \"scan\" block needs scan=(nx, ny)")
        nx, ny = int(scan[0]), int(scan[1])
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")  # [ny, nx], as the scan itself is laid out
        scan_p = ((ny - 1 - iy) * nx + ix).reshape(-1), (iy * nx + (nx - 1 - ix)).reshape(-1)
    for blk in layout:
        for m, (jp, js) in enumerate(((lrp, lrs), (fbp, fbs))):
            if blk == "joint":
                perms[m] += list(off + jp)
                signs[m] += list(js)
            elif blk == "scan":
                perms[m] += list(off + scan_p[m])
                signs[m] += [1.0] * (nx * ny)
            else:
                perms[m] += [off, off + 1, off + 2]
                signs[m] += list(_VEC[blk][m])
        off += len(joint_names) if blk == "joint" else (nx * ny if blk == "scan" else 3)
    ident = np.arange(off)
    lr_p, fb_p = np.array(perms[0]), np.array(perms[1])
    lr_s, fb_s = np.array(signs[0], dtype=np.float64), np.array(signs[1], dtype=np.float64)
    # diagonal: y = FB(LR(x)) -> y[c] = fb_s[c] * lr_s[fb_p[c]] * x[lr_p[fb_p[c]]]
    perm = np.stack([ident, lr_p, fb_p, lr_p[fb_p]]).astype(np.int32)
    sign = np.stack([np.ones(off), lr_s, fb_s, fb_s * lr_s[fb_p]]).astype(np.float32)
    return perm, sign


# the policy observation of the velocity tasks (anymal.py:110-125): angular velocity, projected gravity, command, q, qd, last action
POLICY_LAYOUT = ("ang", "lin", "cmd", "joint", "joint", "joint")
ACTION_LAYOUT = ("joint",)


# the block of every observation term kind of the env descriptor (desc.OBS_KINDS)
KIND_BLOCK = dict(base_lin_vel="lin", base_ang_vel="ang", projected_gravity="lin", generated_commands="cmd", joint_pos_rel="joint",
                  joint_pos_rel_without_wheel="joint", joint_vel_rel="joint", last_action="joint", height_scan="scan")


def _check_table(name, table, n_sym=None):
    perm, sign = table
    perm, sign = np.ascontiguousarray(perm), np.ascontiguousarray(sign, dtype=np.float32)
    if perm.ndim != 2 or perm.shape != sign.shape or not np.issubdtype(perm.dtype, np.integer):
        raise ValueError(f"SymmetryTables: {name}: perm (integer) and sign must both be [n_sym, dim], got {perm.shape} {perm.dtype} and {sign.shape}")
    perm = perm.astype(np.int32)
    ns, dim = perm.shape
    if not 1 <= ns <= MAX_SYM:
        raise ValueError(f"SymmetryTables: {name}: n_sym = {ns} outside 1..{MAX_SYM}")
    if n_sym is not None and ns != n_sym:
        raise ValueError(f"SymmetryTables: {name}: {ns} copies where the observation table has {n_sym}")
    for s in range(ns):
        seen = np.zeros(dim, dtype=bool)
        for c in range(dim):
            src, sg = int(perm[s, c]), float(sign[s, c])
            if not 0 <= src < dim:
                raise ValueError(f"SymmetryTables: {name}: copy {s}, column {c}: source column {src} outside 0..{dim - 1}")
            if seen[src]:
                raise ValueError(f"SymmetryTables: {name}: copy {s}, column {c}: source column {src} is used twice (the row is not a bijection)")
            seen[src] = True
            if sg not in (1.0, -1.0):
                raise ValueError(f"SymmetryTables: {name}: copy {s}, column {c}: sign {sg} is not +1 or -1")
            if s == 0 and (src != c or sg != 1.0):
                raise ValueError(f"SymmetryTables: {name}: copy 0, column {c}: copy 0 must be the identity")
    perm.setflags(write=False)
    sign.setflags(write=False)
    return perm, sign


@dataclasses.dataclass(frozen=True)
class SymmetryTables:
    """The signed column permutations of a symmetry augmentation: `obs`, `critic`, `act` = (perm int32 [n_sym, dim],
    sign float32 [n_sym, dim]); copy s of a row x is sign[s] * x[perm[s]], copy 0 the identity.  `critic=None`: the critic's
    observations are replicated unchanged (what the reference does to every group but "policy", anymal.py:52).
    Checked on construction (the learners index device memory with them); `check_widths` is called by the learners."""
    obs: tuple
    critic: tuple | None
    act: tuple

    def __post_init__(self):
        obs = _check_table("obs", self.obs)
        object.__setattr__(self, "obs", obs)
        object.__setattr__(self, "act", _check_table("act", self.act, obs[0].shape[0]))
        if self.critic is not None:
            object.__setattr__(self, "critic", _check_table("critic", self.critic, obs[0].shape[0]))

    @property
    def n_sym(self) -> int:
        return int(self.obs[0].shape[0])

    def check_widths(self, obs_dim, critic_dim, act_dim):
        for name, t, want in (("obs", self.obs, obs_dim), ("critic", self.critic, critic_dim), ("act", self.act, act_dim)):
            if t is not None and t[0].shape[1] != want:
                raise ValueError(f"SymmetryTables: {name}: the table has {t[0].shape[1]} columns, the network's {name} width is {want}")
        return self

    def __repr__(self):
        return (f"SymmetryTables(n_sym={self.n_sym}, obs={self.obs[0].shape[1]}, "
                f"critic={'replicated' if self.critic is None else self.critic[0].shape[1]}, act={self.act[0].shape[1]})")


def parse_mirrors(mirrors):
    """"lr" | "fb" | "lr,fb" | ("lr", "fb") -> a tuple in the order (lr, fb)"""
    m = tuple(x.strip() for x in mirrors.split(",")) if isinstance(mirrors, str) else tuple(mirrors)
    if not m or len(set(m)) != len(m) or any(x not in ("lr", "fb") for x in m):
        raise ValueError(f"mirrors must be a non-empty subset of (\"lr\", \"fb\"), not {mirrors!r}")
    return tuple(x for x in ("lr", "fb") if x in m)


def expand_history(table, term_dims, hist):
    """A per-FRAME signed permutation `table` = (perm [n_sym, frame_dim], sign [n_sym, frame_dim]) -> the one of the term-major
    history row of an env with observation history (`rl_env_set_obs_history`): term k of width `term_dims[k]` owns
    max(hist[k], 1) frames side by side, oldest first, and a mirror acts on every frame slot alike - column j of slot s of term k takes
    column perm[j] of slot s of the same term.  Raises if a copy moves a column out of its term's block (a history row keeps no place for it)."""
    perm, sign = np.asarray(table[0]), np.asarray(table[1])
    term_dims, hist = [int(d) for d in term_dims], [max(1, int(h)) for h in hist]
    if len(term_dims) != len(hist):
        raise ValueError(f"expand_history: {len(hist)} history lengths for {len(term_dims)} terms")
    if perm.ndim != 2 or perm.shape != sign.shape or perm.shape[1] != sum(term_dims):
        raise ValueError(f"expand_history: the table has shape {perm.shape}, the terms add up to {sum(term_dims)} columns")
    out_p, out_s = [], []
    foff = hoff = 0
    for k, (d, H) in enumerate(zip(term_dims, hist)):
        p = perm[:, foff:foff + d] - foff
        if ((p < 0) | (p >= d)).any():
            s, j = np.argwhere((p < 0) | (p >= d))[0]
            raise ValueError(f"expand_history: copy {s} maps column {foff + j} (term {k}) to column {int(perm[s, foff + j])} outside the term's "
                             f"block {foff}..{foff + d - 1}: a permutation that crosses term blocks has no history form")
        for s in range(H):
            out_p.append(hoff + s * d + p)
            out_s.append(sign[:, foff:foff + d])
        foff += d
        hoff += H * d
    return np.concatenate(out_p, axis=1).astype(np.int32), np.concatenate(out_s, axis=1).astype(np.float32)


def tables_for_env(env_or_desc, mirrors=("lr",)) -> SymmetryTables:
    """`SymmetryTables` of a velocity task from its descriptor (`env.desc`): the joint names give the per-joint mirrors, the
    `task.policy` / `task.critic` term lists the layout of the two observation rows (the height scan's grid from
    `task.scan_nx / scan_ny`), actions are one column per DOF in joint order.  `mirrors`: ("lr",) -> identity + left-right;
    ("fb",) -> identity + front-back; both -> the reference's four copies (identity, lr, fb, fb o lr).
    Note on "fb": it is the reference's rule (pitch joints flip), exact for a robot whose nominal pose is front-back
    symmetric (ANYmal's X configuration); the Unitree quadrupeds bend all four knees backward, so for them it is a
    regulariser rather than a symmetry of the dynamics.  "lr" is exact for all of them."""
    from .desc import OBS_KINDS

    desc = getattr(env_or_desc, "desc", env_or_desc)
    mirrors = parse_mirrors(mirrors)
    names = list(desc.joint_names)[:desc.model.num_dof]
    kw = None
    for style in (UNITREE, {}):  # ({}: joint_tables' defaults, ANYmal)
        try:
            joint_tables(names, **style)
            kw = style
            break
        except (ValueError, KeyError):  # a name that does not parse / a leg without its mirror partner
            pass
    if kw is None or len(names) != desc.model.num_dof:
        raise ValueError(f"tables_for_env: the joint names {names[:4]}... parse neither as Unitree-style (FR_hip_joint) nor as ANYmal-style (LF_HAA) "
                         "legs: no mirror tables can be derived for this robot (humanoids, Tita); pass explicit SymmetryTables(obs, critic, act) instead")
    t = desc.task
    scan = (int(t.scan_nx), int(t.scan_ny))
    rows = [0] + [dict(lr=1, fb=2)[m] for m in mirrors] + ([3] if len(mirrors) == 2 else [])

    def table(layout):
        perm, sign = layout_tables(layout, names, scan=scan if "scan" in layout else None, **kw)
        return perm[rows], sign[rows]

    hist = getattr(env_or_desc, "obs_history", None) or {}  # an env with observation history: the same mirror in every frame slot

    def group(terms, n, g):
        tab = table(tuple(KIND_BLOCK[OBS_KINDS[terms[i].kind]] for i in range(n)))
        lengths = hist.get(("policy", "critic")[g]) if isinstance(hist, dict) else None
        return expand_history(tab, desc.obs_term_dims(g), lengths) if lengths else tab

    return SymmetryTables(obs=group(t.policy, t.n_policy, 0), critic=group(t.critic, t.n_critic, 1), act=table(ACTION_LAYOUT))


class SymmetryAugmentation:
    """`aug(x)`: [n, dim] device tensor -> [n_sym * n, dim] (copy s in rows s * n .. (s + 1) * n)."""

    def __init__(self, perm, sign, device: str = "cuda:0", lib_path: str | None = None):
        import torch

        self._torch = torch
        self.lib = load_rollout_library(lib_path)
        self.lib.rl_symmetry_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_void_p)]
        self.lib.rl_symmetry_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        self.lib.rl_symmetry_destroy.argtypes = [C.c_void_p]
        self.device = torch.device(device)
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        sign = np.ascontiguousarray(sign, dtype=np.float32)
        if perm.shape != sign.shape or perm.ndim != 2:
            raise ValueError("perm and sign must both be [n_sym, dim]")
        self.n_sym, self.dim = perm.shape
        self.handle = C.c_void_p()
        if self.lib.rl_symmetry_create(self.n_sym, self.dim, perm.ctypes.data_as(C.POINTER(C.c_int32)), sign.ctypes.data_as(C.POINTER(C.c_float)),
                                       self.device.index or 0, C.byref(self.handle)) != 0:
            raise RlRolloutError((self.lib.rl_rollout_last_error() or b"").decode())

    def __call__(self, x):
        torch = self._torch
        if x.dtype != torch.float32 or not x.is_contiguous() or x.ndim != 2 or x.shape[1] != self.dim or x.device != self.device:
            raise RlRolloutError(f"expected a contiguous fp32 [n, {self.dim}] tensor on {self.device}")
        out = torch.empty((self.n_sym * x.shape[0], self.dim), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if self.lib.rl_symmetry_apply(self.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.shape[0], stream) != 0:
            raise RlRolloutError((self.lib.rl_rollout_last_error() or b"").decode())
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rl_symmetry_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


_cache: dict = {}


def compute_symmetric_states(env, obs=None, actions=None):
    """Drop-in for the reference function (same signature and return value): `obs` is a dict / TensorDict with a
    "policy" entry (other groups are replicated unchanged, anymal.py:52), `actions` a [n, 12] tensor."""
    import torch

    def aug(x, layout):
        key = (layout, str(x.device))
        if key not in _cache:
            _cache[key] = SymmetryAugmentation(*layout_tables(layout), device=str(x.device))
        return _cache[key](x.contiguous().float())

    obs_aug = act_aug = None
    if obs is not None:
        obs_aug = type(obs)({k: (aug(v, POLICY_LAYOUT) if k == "policy" else v.repeat(4, *([1] * (v.ndim - 1)))) for k, v in obs.items()})
    if actions is not None:
        act_aug = aug(actions, ACTION_LAYOUT)
    return obs_aug, act_aug
