"""Symmetry data augmentation inside the PPO update, CPU tier: the tables `symmetry.tables_for_env` derives for the robots this project
runs (by joint NAME and grid position, never by comparing the builder with itself), the checks of `symmetry.SymmetryTables`, and the rule
of `ppo.PPO(symmetry=...)` against the materialised construction: today's plain `PPO.update` on a storage that holds the n_sym n rows
(mirrored observations and actions, every other term repeated), one epoch of one mini-batch.  The HIP learner's half is
tests/test_gpu_ppo_hip_symmetry.py."""
import copy
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

from ppo_helpers import fake_storage, random_table as _random_table
from robot_lab_amd.desc import OBS_KINDS, arr
from robot_lab_amd.ppo import PPO, ActorCritic, gaussian_kl
from robot_lab_amd.scene import load_bundle
from robot_lab_amd.symmetry import _VEC, SymmetryTables, tables_for_env

TASK = "RobotLab-Isaac-Velocity-{}-v0"


def _desc(name):
    return load_bundle(TASK.format(name))[0]


def _offsets(desc, group):
    """{term kind: first column} of an observation row, from the descriptor's term list"""
    t = desc.task
    terms, n = (t.policy, t.n_policy) if group == "policy" else (t.critic, t.n_critic)
    D = desc.model.num_dof
    width = {k: 3 for k in ("base_lin_vel", "base_ang_vel", "projected_gravity", "generated_commands")}
    width.update({k: D for k in ("joint_pos_rel", "joint_pos_rel_without_wheel", "joint_vel_rel", "last_action")}, height_scan=t.scan_nx * t.scan_ny)
    out, off = {}, 0
    for i in range(n):
        kind = OBS_KINDS[terms[i].kind]
        out[kind] = off
        off += width[kind]
    return out, off


def _joint_map(desc, perm, sign, off=0):
    """{joint name: (name of the joint it reads, sign)} of one copy of a per-joint block that starts at column `off`"""
    names = list(desc.joint_names)
    return {n: (names[int(perm[off + j]) - off], float(sign[off + j])) for j, n in enumerate(names)}


@pytest.mark.parametrize("robot", ["Rough-Unitree-A1", "Rough-Unitree-Go2W"])
def test_tables_by_joint_name_and_grid_position(robot):
    desc = _desc(robot)
    tab = tables_for_env(desc, ("lr", "fb"))  # copies: identity, lr, fb, fb o lr
    D = desc.model.num_dof
    pol, pol_w = _offsets(desc, "policy")
    cri, cri_w = _offsets(desc, "critic")
    assert tab.n_sym == 4 and tab.act[0].shape == (4, D) and tab.obs[0].shape == (4, pol_w) and tab.critic[0].shape == (4, cri_w)
    if robot == "Rough-Unitree-A1":
        assert (pol_w, cri_w, D) == (45, 235, 12)
    wheeled = "FR_foot_joint" in desc.joint_names
    assert wheeled == (robot == "Rough-Unitree-Go2W")
    # the per-joint blocks: actions, and q / qd / last action inside both observation rows
    blocks = [(tab.act, 0)] + [(tab.obs, pol[k]) for k in pol if k.startswith("joint") or k == "last_action"] + \
             [(tab.critic, cri[k]) for k in cri if k.startswith("joint") or k == "last_action"]
    assert len(blocks) == 7
    for (perm, sign), off in blocks:
        lr, fb = _joint_map(desc, perm[1], sign[1], off), _joint_map(desc, perm[2], sign[2], off)
        assert lr["FR_hip_joint"] == ("FL_hip_joint", -1.0) and lr["FL_hip_joint"] == ("FR_hip_joint", -1.0) and lr["RL_hip_joint"] == ("RR_hip_joint", -1.0)
        assert lr["FR_thigh_joint"] == ("FL_thigh_joint", 1.0) and lr["RL_calf_joint"] == ("RR_calf_joint", 1.0)
        assert fb["FR_hip_joint"] == ("RR_hip_joint", 1.0) and fb["RL_thigh_joint"] == ("FL_thigh_joint", -1.0) and fb["FL_calf_joint"] == ("RL_calf_joint", -1.0)
        if wheeled:  # a wheel's spin is the y component of an axial vector: normal to the left-right plane (+1), inside the front-back plane (-1)
            assert lr["FR_foot_joint"] == ("FL_foot_joint", 1.0) and lr["RL_foot_joint"] == ("RR_foot_joint", 1.0)
            assert fb["FR_foot_joint"] == ("RR_foot_joint", -1.0) and fb["RL_foot_joint"] == ("FL_foot_joint", -1.0)
    # the 3-vectors stay in place and take the signs of _VEC
    vec = dict(base_lin_vel="lin", base_ang_vel="ang", projected_gravity="lin", generated_commands="cmd")
    assert "base_lin_vel" in cri and "base_lin_vel" not in pol
    for (perm, sign), offs in ((tab.obs, pol), (tab.critic, cri)):
        for kind, blk in vec.items():
            if kind in offs:
                o = offs[kind]
                for copy_, m in ((1, 0), (2, 1)):
                    assert list(perm[copy_, o:o + 3]) == [o, o + 1, o + 2] and tuple(sign[copy_, o:o + 3]) == _VEC[blk][m], (kind, copy_)
    # the height scan: column iy * nx + ix
    nx, ny, o = desc.task.scan_nx, desc.task.scan_ny, cri["height_scan"]
    assert (nx, ny) == (17, 11) and o + nx * ny == cri_w
    perm, sign = tab.critic
    for ix in range(nx):
        for iy in range(ny):
            c = o + iy * nx + ix
            assert perm[1, c] == o + (ny - 1 - iy) * nx + ix and perm[2, c] == o + iy * nx + (nx - 1 - ix) and perm[3, c] == o + (ny - 1 - iy) * nx + (nx - 1 - ix)
    assert (sign[:, o:] == 1).all()


def _apply(table, s, x):
    return table[1][s] * x[..., table[0][s]]


def test_table_properties():
    rng = np.random.default_rng(0)
    for robot in ("Rough-Unitree-A1", "Rough-Unitree-Go2", "Rough-Unitree-Go2W", "Flat-Unitree-B2"):
        desc = _desc(robot)
        tab = tables_for_env(desc, ("lr", "fb"))
        for table in (tab.obs, tab.critic, tab.act):
            x = rng.standard_normal((5, table[0].shape[1])).astype(np.float32)
            for s in range(4):  # every mirror, and the product of the two, is an involution
                np.testing.assert_array_equal(_apply(table, s, _apply(table, s, x)), x)
            np.testing.assert_array_equal(_apply(table, 3, x), _apply(table, 2, _apply(table, 1, x)))  # copy 3 = fb o lr ...
            np.testing.assert_array_equal(_apply(table, 2, _apply(table, 1, x)), _apply(table, 1, _apply(table, 2, x)))  # ... = lr o fb
        only_lr, only_fb = tables_for_env(desc), tables_for_env(desc, "fb")
        assert only_lr.n_sym == 2 and only_fb.n_sym == 2
        np.testing.assert_array_equal(only_lr.critic[0], tab.critic[0][[0, 1]])
        np.testing.assert_array_equal(only_fb.act[1], tab.act[1][[0, 2]])
        assert tables_for_env(desc, "lr,fb").n_sym == 4 and tables_for_env(desc, ("fb", "lr")).obs[0].tolist() == tab.obs[0].tolist()
    for robot in ("Rough-Unitree-A1", "Rough-Unitree-Go2"):  # the nominal pose is left-right symmetric
        desc = _desc(robot)
        q0 = arr(desc.model.default_joint_pos, desc.model.num_dof).copy()
        assert np.abs(q0).max() > 0.5
        np.testing.assert_array_equal(_apply(tables_for_env(desc).act, 1, q0), q0)
    with pytest.raises(ValueError, match="SymmetryTables"):  # the message names the way out
        tables_for_env(_desc("Rough-Unitree-G1"))
    with pytest.raises(ValueError, match="mirrors"):
        tables_for_env(_desc("Rough-Unitree-A1"), ("lr", "diag"))


def _ident(n_sym, dim):
    return np.tile(np.arange(dim, dtype=np.int32), (n_sym, 1)), np.ones((n_sym, dim), dtype=np.float32)


def test_symmetry_tables_validation():
    ok = SymmetryTables(obs=_ident(2, 5), critic=None, act=_ident(2, 3))
    assert ok.n_sym == 2 and ok.critic is None and ok.obs[0].dtype == np.int32 and ok.obs[1].dtype == np.float32 and "replicated" in repr(ok)
    with pytest.raises(dataclasses.FrozenInstanceError):
        ok.obs = _ident(2, 5)
    p, s = _ident(2, 5)
    p[1] = [1, 0, 2, 2, 4]
    with pytest.raises(ValueError, match=r"obs: copy 1, column 3: source column 2 is used twice"):
        SymmetryTables(obs=(p, s), critic=None, act=_ident(2, 3))
    p, s = _ident(2, 5)
    s[1, 4] = 0.5
    with pytest.raises(ValueError, match=r"critic: copy 1, column 4: sign 0.5"):
        SymmetryTables(obs=_ident(2, 4), critic=(p, s), act=_ident(2, 3))
    p, s = _ident(2, 3)
    p[0] = [1, 0, 2]
    with pytest.raises(ValueError, match=r"act: copy 0, column 0: copy 0 must be the identity"):
        SymmetryTables(obs=_ident(2, 4), critic=None, act=(p, s))
    p, s = _ident(2, 3)
    s[0, 2] = -1
    with pytest.raises(ValueError, match=r"act: copy 0, column 2: copy 0 must be the identity"):
        SymmetryTables(obs=_ident(2, 4), critic=None, act=(p, s))
    with pytest.raises(ValueError, match=r"n_sym = 9 outside 1..8"):
        SymmetryTables(obs=_ident(9, 4), critic=None, act=_ident(9, 3))
    with pytest.raises(ValueError, match=r"act: 3 copies where the observation table has 2"):
        SymmetryTables(obs=_ident(2, 4), critic=None, act=_ident(3, 3))
    with pytest.raises(ValueError, match=r"must both be \[n_sym, dim\]"):
        SymmetryTables(obs=(_ident(2, 4)[0], _ident(2, 5)[1]), critic=None, act=_ident(2, 3))
    with pytest.raises(ValueError, match=r"critic: the table has 5 columns, the network's critic width is 7"):
        SymmetryTables(obs=_ident(2, 4), critic=_ident(2, 5), act=_ident(2, 3)).check_widths(4, 7, 3)
    pol = ActorCritic(4, 7, 3, actor_hidden=(8,), critic_hidden=(8,))
    with pytest.raises(ValueError, match=r"obs: the table has 5 columns, the network's obs width is 4"):
        PPO(pol, symmetry=ok)
    with pytest.raises(TypeError, match="SymmetryTables"):
        PPO(pol, symmetry="lr")


# ---- the rule against the materialised construction ------------------------------------------------------------------------------------
T, N, OD, CD, A, NSYM = 4, 24, 45, 235, 12, 3
ROWS = T * N  # 96
_fake_storage = functools.partial(fake_storage, T=T, N=N, od=OD, cd=CD, A=A, dtype=torch.float64)


def _materialise(st, tab):
    """the storage of n_sym * rows rows the rule is defined by: copy s of every row in rows s * rows .. (s + 1) * rows, as a 1 x (n_sym rows) storage"""
    ns = tab.n_sym
    rows = st.num_transitions_per_env * st.num_envs
    flat = lambda t: t.reshape(rows, -1)  # noqa: E731

    def mirrored(x, table):
        if table is None:
            return flat(x).repeat(ns, 1)
        perm, sign = torch.as_tensor(table[0].astype(np.int64)), torch.as_tensor(table[1].copy()).to(x.dtype)
        return torch.cat([sign[s] * flat(x)[:, perm[s]] for s in range(ns)], 0)

    out = types.SimpleNamespace(num_transitions_per_env=1, num_envs=ns * rows)
    out.observations, out.privileged_observations, out.actions = mirrored(st.observations, tab.obs), mirrored(st.privileged_observations, tab.critic), mirrored(st.actions, tab.act)
    for k in ("values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
        setattr(out, k, flat(getattr(st, k)).repeat(ns, 1))
    for k, v in list(vars(out).items()):
        if torch.is_tensor(v):
            setattr(out, k, v.unsqueeze(0))
    return out


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(0)
    pol = ActorCritic(OD, CD, A).double()
    st = _fake_storage(pol)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # perturbed, so that the probability ratio of the stored rows is not 1
        for p in pol.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g, dtype=torch.float64) * p.abs().mean())
    return pol, st


@pytest.mark.parametrize("critic_table", [True, False])
def test_rule_equals_the_plain_update_on_the_materialised_rows(case, critic_table):
    pol, st = case
    rng = np.random.default_rng(7)
    tab = SymmetryTables(obs=_random_table(rng, NSYM, OD), critic=_random_table(rng, NSYM, CD) if critic_table else None, act=_random_table(rng, NSYM, A))
    kw = dict(num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30)
    sym = PPO(copy.deepcopy(pol), symmetry=tab, **kw)
    s_sym = sym.update(st, torch.Generator().manual_seed(3))
    mat = PPO(copy.deepcopy(pol), **kw)  # today's update, no symmetry: the comparator
    s_mat = mat.update(_materialise(st, tab), torch.Generator().manual_seed(4))
    for (n, p), (_, q) in zip(sym.policy.named_parameters(), mat.policy.named_parameters()):
        scale = q.grad.abs().max().item()
        assert scale > 0
        err = (p.grad - q.grad).abs().max().item() / scale
        assert err <= 1e-12, (n, err)
    for k in ("value_loss", "surrogate_loss", "entropy"):  # means over the n_sym n rows
        assert abs(s_sym[k] - s_mat[k]) <= 1e-12 * abs(s_mat[k]), (k, s_sym[k], s_mat[k])
    # the KL statistic: the 96 stored rows only, against their stored mu / sigma
    with torch.no_grad():
        mean, std = pol.distribution(st.observations.reshape(ROWS, OD))
        kl = float(gaussian_kl(st.mu.reshape(ROWS, A), st.sigma.reshape(ROWS, A), mean, std).mean())
    assert kl > 0 and abs(s_sym["kl"] - kl) <= 1e-12 * kl, (s_sym["kl"], kl)
    assert abs(s_mat["kl"] - kl) > 1e-3 * kl  # (the materialised run's statistic averages the copies too: the rule's KL is NOT that)


def test_symmetry_none_is_the_learner_without_the_keyword(case):
    pol, st = case
    a, b = PPO(copy.deepcopy(pol)), PPO(copy.deepcopy(pol), symmetry=None)
    sa, sb = a.update(st, torch.Generator().manual_seed(5)), b.update(st, torch.Generator().manual_seed(5))
    assert sa == sb
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)


def test_identity_tables_are_the_plain_update(case):
    """n_sym = 1 (the identity alone) is the plain update, bit for bit"""
    pol, st = case
    a = PPO(copy.deepcopy(pol))
    b = PPO(copy.deepcopy(pol), symmetry=SymmetryTables(obs=_ident(1, OD), critic=_ident(1, CD), act=_ident(1, A)))
    sa, sb = a.update(st, torch.Generator().manual_seed(5)), b.update(st, torch.Generator().manual_seed(5))
    assert sa == sb
    for p, q in zip(a.policy.parameters(), b.policy.parameters()):
        assert torch.equal(p, q)
