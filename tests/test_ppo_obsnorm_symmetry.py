"""Observation normalisation TOGETHER WITH symmetry, CPU tier: the rule of `ppo.PPO(symmetry=...)` on a policy with normalisers over the RAW
storage - mirror the raw row, then normalise it with the statistics of the destination column - against the unchanged plain `ppo.PPO` on an
identity-normaliser copy of the policy over the materialised rows; that the ORDER can be seen with asymmetric statistics (the teeth); and the
seeds the GPU tests of tests/test_gpu_ppo_hip_obsnorm.py rely on.  Setup: tests/obsnorm_symmetry_helpers.py.  Comparison and tolerance are
those of tests/test_ppo_symmetry.py (relative gradient error per tensor <= 1e-12 in fp64, one epoch of one mini-batch, no clipping)."""
import copy

import pytest
import torch

import obsnorm_symmetry_helpers as H
from ppo_helpers import cast, torch_learner
from robot_lab_amd.ppo import PPO

TOL = 1e-12
ROWS = 96  # as tests/test_ppo_symmetry.py: the first 96 rows of the flat batch
KW = dict(num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30)


def _sub(st, rows, dtype):
    """the first `rows` rows of the flat batch as a 1 x rows storage in `dtype` on the host"""
    return cast(st, dtype, rows=torch.arange(rows), device="cpu")


def _errors(a, b):
    """{tensor: max |grad a - grad b| / max |grad b|}"""
    out = {}
    for (n, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
        scale = q.grad.abs().max().item()
        assert scale > 0, n
        out[n] = (p.grad - q.grad).abs().max().item() / scale
    return out


def _mirror_term(policy, mat, tab, n):
    """L_mirror from the formula on the materialised network inputs `mat` (copy s in rows s n .. (s + 1) n): `policy`'s .grad fields are then
    those of L_mirror alone (as tests/test_ppo_mirror_loss.py)"""
    x = mat.observations.reshape(tab.n_sym * n, -1)
    mu = policy.actor(x)
    tau = H.mirrored(mu[:n].detach(), tab.act, tab.n_sym)
    return ((mu[n:] - tau[n:]) ** 2).sum() / ((tab.n_sym - 1) * n * mu.shape[1])


@pytest.mark.parametrize("name", list(H.CASES))
@pytest.mark.parametrize("critic_table", [True, False], ids=["critic-mirrored", "critic-replicated"])
def test_rule_mirrors_the_raw_row_then_normalises(name, critic_table):
    """`PPO(symmetry=tab, ...)` with normalisers on raw rows == the unchanged plain `PPO` on identity normalisers over the mirror-then-normalise rows
    (without the augmentation: over the normalised stored rows), plus - under a mirror loss - coeff x the gradient of L_mirror from its formula
    on the same materialised rows"""
    case_kw = H.CASES[name]
    pol, st = H.case()
    tab = H._tables(3, critic_table)
    p64 = copy.deepcopy(pol).double()
    raw, idx = _sub(st, ROWS, torch.float64), torch.arange(ROWS)
    sym = PPO(copy.deepcopy(p64), symmetry=tab, **KW, **case_kw)
    s_sym = sym.update(raw, torch.Generator().manual_seed(3))
    mat = H.materialise(raw, tab, idx, p64)
    plain = PPO(H.without_normalizers(p64), **KW)  # the unchanged plain update, no symmetry, no normaliser: the comparator
    s_plain = plain.update(mat if case_kw.get("data_augmentation", True) else H.materialise(raw, None, idx, p64), torch.Generator().manual_seed(4))
    mir, coeff = H.without_normalizers(p64), case_kw.get("mirror_loss", 0.0)
    if coeff:
        L = _mirror_term(mir, mat, tab, ROWS)
        L.backward()
        L = float(L.detach())
        assert L > 0 and abs(s_sym["mirror_loss"] - L) <= TOL * L
    err = {}
    for (n, p), (_, q), (_, m) in zip(sym.policy.named_parameters(), plain.policy.named_parameters(), mir.named_parameters()):
        want = q.grad + (coeff * m.grad if m.grad is not None else 0.0)
        scale = want.abs().max().item()
        assert scale > 0, n
        err[n] = (p.grad - want).abs().max().item() / scale
    print({n: f"{e:.1e}" for n, e in err.items()})
    assert max(err.values()) <= TOL, err
    for k in ("value_loss", "surrogate_loss", "entropy"):
        assert abs(s_sym[k] - s_plain[k]) <= TOL * abs(s_plain[k]), (k, s_sym[k], s_plain[k])


def test_the_order_can_be_seen():
    """Teeth: normalise first, then mirror - what a learner does that mirrors behind a normalisation pass - misses the tolerance of the test above
    by many orders of magnitude with these statistics (measured on this batch: between 0.43 and 630 relative gradient error per tensor against 1e-12, eleven orders of magnitude and more)."""
    pol, st = H.case()
    tab = H._tables(3)
    p64 = copy.deepcopy(pol).double()
    raw = _sub(st, ROWS, torch.float64)
    sym = PPO(copy.deepcopy(p64), symmetry=tab, **KW)
    sym.update(raw, torch.Generator().manual_seed(3))
    wrong = PPO(H.without_normalizers(p64), **KW)
    wrong.update(H.materialise(raw, tab, torch.arange(ROWS), p64, order="normalise-then-mirror"), torch.Generator().manual_seed(4))
    err = _errors(sym, wrong)
    print({n: f"{e:.1e}" for n, e in err.items()})
    assert min(err.values()) > 1e6 * TOL, err  # every tensor, the output layers included


def test_without_symmetry_the_rule_is_the_modules_forward():
    """no symmetry: `PPO` on raw rows == `PPO` on identity normalisers over the normalised rows (`y = (o - mean) / (std + eps)`)"""
    pol, st = H.case()
    p64 = copy.deepcopy(pol).double()
    raw = _sub(st, ROWS, torch.float64)
    a = PPO(copy.deepcopy(p64), **KW)
    a.update(raw, torch.Generator().manual_seed(3))
    b = PPO(H.without_normalizers(p64), **KW)
    b.update(H.materialise(raw, None, torch.arange(ROWS), p64), torch.Generator().manual_seed(3))
    err = _errors(a, b)
    assert max(err.values()) <= TOL, err


@pytest.mark.parametrize("name", list(H.CASES))
def test_pinned_seeds_give_one_learning_rate_path(name):
    """with PERTURB_SEED / UPDATE_SEED and DESIRED_KL the fp64 and the fp32 torch learner walk the same 20-step learning-rate path under TABLES(2):
    the GPU tests' `identical learning-rate path` and Adam-displacement bounds rely on it.  The path has teeth: it rises, holds and falls."""
    pol, st = H.case()
    tab = H._tables(2)
    paths = []
    for dtype in (torch.float64, torch.float32):
        alg = torch_learner(pol, dtype, device="cpu", symmetry=tab, desired_kl=H.DESIRED_KL, **H.CASES[name])
        alg.update(cast(st, dtype, device="cpu"), torch.Generator().manual_seed(H.UPDATE_SEED))
        paths.append(alg.lr_path)
    assert len(paths[0]) == 20 and paths[0] == paths[1], paths
    steps = [b / a for a, b in zip(paths[0], paths[0][1:])]
    assert any(s > 1 for s in steps) and any(s < 1 for s in steps) and sum(s == 1 for s in steps) >= 3, paths[0]


def test_trainer_keywords():
    import inspect

    from robot_lab_amd.ppo import Trainer
    from robot_lab_amd.ppo_hip import HipPPO

    assert inspect.signature(Trainer.__init__).parameters["normalize_in_learner"].default is False
    assert inspect.signature(HipPPO.__init__).parameters["obs_normalizers"].default is None
