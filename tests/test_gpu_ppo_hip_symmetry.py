"""`-m gpu`: symmetry data augmentation inside the HIP PPO learner (`rl_ppo_set_symmetry`, the SYM instantiations of csrc/rl_ppo.hip,
`ppo_hip.HipPPO(symmetry=...)`) against the torch learner of robot_lab_amd/ppo.py.

Setup as tests/test_gpu_ppo_hip.py: ActorCritic(45, 235, 12), a `_fake_storage` with T = 24, N = 256, parameters perturbed.  The tables are
random signed permutations drawn here from a seeded generator (row 0 the identity): arbitrary gathers, and nothing of symmetry.py's builders
enters the kernel check.  Comparators, never the code under test:
  gradients  the UNCHANGED `ppo.PPO` (no symmetry) in fp64 on the materialised rows - the n_sym n rows written out, mirrored observations and
             actions, everything else repeated - one epoch of one mini-batch; the same in fp32 measures what fp32 round-off alone does (d)
  update     `ppo.PPO(symmetry=...)` in fp64 (its rule is pinned to the materialised construction by tests/test_ppo_symmetry.py), fp32 for the margin
Bounds: those of tests/test_gpu_ppo_hip.py (e <= 8 d per tensor; q999 <= max(8 q999_32, ulp), max <= sum of the learning rates), with the same
`ulp` idea as a floor of the gradient bound: one fp32 spacing of the tensor's largest fp64 gradient entry, relative to that entry - below it
an fp32 result cannot be told from the fp64 one, whatever d happens to be."""
import copy
import functools
import types

import numpy as np
import pytest

from ppo_helpers import DEV, cast as _cast, fake_storage as _fake_storage, gen as _gen, perm as perm_of, split as _split, tables, torch_learner as _torch_learner

pytestmark = pytest.mark.gpu

T, N, OD, CD, A = 24, 256, 45, 235, 12
B, MB = T * N, T * N // 4
_perm, _tables = functools.partial(perm_of, B), functools.partial(tables, (OD, CD, A))
PERTURB_SEED = 1  # with it the fp64 and the fp32 torch learner walk the same 20-step learning-rate path under TABLES(2) (asserted below)


def _materialise(st, tab, idx):
    """the n_sym * len(idx) rows the rule is defined by, as a 1 x rows storage (`st`: a `_cast` storage; copy s in rows s n .. (s + 1) n)"""
    import torch

    ns = tab.n_sym
    rows = lambda t: t.reshape(B, -1)[idx]  # noqa: E731

    def mirrored(x, table):
        x = rows(x)
        if table is None:
            return x.repeat(ns, 1)
        perm, sign = torch.as_tensor(table[0].astype(np.int64), device=DEV), torch.as_tensor(table[1].copy(), device=DEV).to(x.dtype)
        return torch.cat([sign[s] * x[:, perm[s]] for s in range(ns)], 0)

    out = types.SimpleNamespace(num_transitions_per_env=1, num_envs=ns * len(idx))
    out.observations, out.privileged_observations, out.actions = mirrored(st.observations, tab.obs), mirrored(st.privileged_observations, tab.critic), mirrored(st.actions, tab.act)
    for k in ("values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
        setattr(out, k, rows(getattr(st, k)).repeat(ns, 1))
    for k, v in list(vars(out).items()):
        if torch.is_tensor(v):
            setattr(out, k, v.unsqueeze(0).contiguous())
    return out


@pytest.fixture(scope="module")
def case():
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pol = ActorCritic(OD, CD, A)
    st = _fake_storage(pol, T, N, OD, CD, A)
    g = torch.Generator().manual_seed(PERTURB_SEED)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g) * p.abs().mean())
    return pol, st


@pytest.mark.parametrize("rows,n_sym,critic", [(1000, 4, True), (37, 2, True), (MB, 2, False)], ids=["1000x4", "37x2", "1536x2-critic-replicated"])
def test_gradient_parity_with_symmetry(case, rows, n_sym, critic):
    """e = max|g_hip - g64| / max|g64| <= max(8 d, one fp32 spacing of max|g64| relative to it), d = max|g32 - g64| / max|g64|, per parameter
    tensor (the table is profiles/ppo_hip_symmetry_grad_parity.txt).  1000 rows x 4 copies: the copy boundaries 1000, 2000, 3000 fall inside a
    128-row tile (1000 = 7 * 128 + 104), inside a 16-row slice (1000 = 62 * 16 + 8) and inside the dW chunks; 37 x 2: everything in one
    partial tile, the boundary at an odd row; 1536 x 2 with `critic=None`: the whole first mini-batch, the critic's rows replicated."""
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    tab = _tables(n_sym, critic)
    idx = _perm()[:rows]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = _torch_learner(pol, dtype, num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30)  # the UNCHANGED update: no symmetry=
        alg.update(_materialise(_cast(st, dtype), tab, idx), _gen(5))
        ref[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}
    hip = HipPPO(copy.deepcopy(pol).to(DEV), max_rows_per_minibatch=MB, symmetry=tab)
    assert "symmetry=SymmetryTables(n_sym=" in repr(hip)
    g_hip = _split(hip.minibatch_grad(_cast(st, torch.float32), idx), pol)
    torch.cuda.synchronize()
    print(f"\n{rows} rows x {n_sym} copies{'' if critic else ', critic replicated'}\n{'tensor':<18}{'max|g64|':>12}{'e (hip)':>12}{'d (torch32)':>13}{'e/d':>8}{'floor':>12}")
    bad = []
    for n, g64 in ref[torch.float64].items():
        scale = g64.abs().max().item()
        e = (g_hip[n].reshape(g64.shape) - g64).abs().max().item() / scale
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        floor = float(np.spacing(np.float32(scale))) / scale
        print(f"{n:<18}{scale:12.4e}{e:12.3e}{d:13.3e}{e / d if d else float('inf'):8.2f}{floor:12.3e}")
        if not e <= max(8 * d, floor):
            bad.append((n, e, d, floor))
    assert not bad, f"gradient error above 8 x the fp32 torch learner's: {bad}"
    hip.close()


def test_one_update_with_symmetry_matches_the_torch_learner(case):
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    tab = _tables(2)
    a64, a32 = _torch_learner(pol, torch.float64, symmetry=tab), _torch_learner(pol, torch.float32, symmetry=tab)
    s64, s32 = a64.update(_cast(st, torch.float64), _gen()), a32.update(_cast(st, torch.float32), _gen())
    assert len(a64.lr_path) == 20 and a64.lr_path == a32.lr_path, "the two torch references took different learning-rate paths: the inputs are mis-chosen"
    hip = HipPPO(copy.deepcopy(pol).to(DEV), symmetry=tab)
    s_hip = hip.update(_cast(st, torch.float32), _gen())
    out = hip.store_into(copy.deepcopy(pol).to(DEV))
    torch.cuda.synchronize()
    p64 = {n: p.detach().double().cpu() for n, p in a64.policy.named_parameters()}
    p32 = {n: p.detach().double().cpu() for n, p in a32.policy.named_parameters()}
    ph = {n: p.detach().double().cpu() for n, p in out.named_parameters()}
    displacement = float(sum(a64.lr_path))  # Adam moves an entry by at most lr per step
    print(f"\n{'tensor':<18}{'q999 hip':>12}{'q999 torch32':>14}{'max hip':>12}{'max torch32':>13}")
    bad = []
    for n in p64:
        dh, d32 = (ph[n] - p64[n]).abs().flatten(), (p32[n] - p64[n]).abs().flatten()
        qh, q32 = torch.quantile(dh, 0.999).item(), torch.quantile(d32, 0.999).item()
        ulp = float(np.spacing(np.float32(p64[n].abs().max().item())))
        print(f"{n:<18}{qh:12.3e}{q32:14.3e}{dh.max().item():12.3e}{d32.max().item():13.3e}")
        if not qh <= max(8 * q32, ulp):
            bad.append((n, "q999", qh, q32))
        if not dh.max().item() <= displacement:
            bad.append((n, "max", dh.max().item(), displacement))
    assert not bad, bad
    print({k: (s_hip[k], s32[k], s64[k]) for k in s64})
    for k in ("value_loss", "surrogate_loss", "entropy", "kl"):
        assert abs(s_hip[k] - s64[k]) <= 8 * abs(s32[k] - s64[k]) + 1e-6 * abs(s64[k]), (k, s_hip[k], s32[k], s64[k])
    assert s_hip["learning_rate"] == s64["learning_rate"] == s32["learning_rate"]
    hip.close()


def test_update_with_symmetry_is_deterministic(case):
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    st32, tab, runs = _cast(st, torch.float32), _tables(3), []
    for _ in range(2):
        hip = HipPPO(copy.deepcopy(pol).to(DEV), symmetry=tab)
        hip.update(st32, _gen())
        runs.append([hip.flat(w).cpu() for w in ("parameters", "exp_avg", "exp_avg_sq")])
        hip.close()
    for x, y in zip(*runs):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_identity_tables_equal_no_symmetry(case):
    """n_sym = 1 runs the SYM instantiations (table words, XOR of a zero sign bit, the KL mask) on one copy: the update without symmetry, bit for bit"""
    import torch

    from robot_lab_amd.ppo_hip import HipPPO
    from robot_lab_amd.symmetry import SymmetryTables

    pol, st = case
    ident = lambda dim: (np.arange(dim, dtype=np.int32)[None], np.ones((1, dim), dtype=np.float32))  # noqa: E731
    st32, runs = _cast(st, torch.float32), []
    for tab in (None, SymmetryTables(obs=ident(OD), critic=ident(CD), act=ident(A))):
        hip = HipPPO(copy.deepcopy(pol).to(DEV), symmetry=tab)
        stats = hip.update(st32, _gen())
        runs.append((stats, [hip.flat(w).cpu() for w in ("parameters", "exp_avg", "exp_avg_sq")]))
        hip.close()
    assert runs[0][0] == runs[1][0]
    for x, y in zip(runs[0][1], runs[1][1]):
        assert torch.equal(x, y)


def test_set_symmetry_refusals(case):
    import torch

    from robot_lab_amd.ppo import ActorCritic
    from robot_lab_amd.ppo_hip import HipPPO, RlPpoError

    pol, st = case
    tab = _tables(2)
    hip = HipPPO(copy.deepcopy(pol).to(DEV), max_rows_per_minibatch=64)
    # the library checks for itself (its table words index device memory), naming table, copy and column; a refused call leaves the handle as it was
    perm = tab.obs[0].copy()
    perm[1, 7] = perm[1, 3]
    with pytest.raises(RlPpoError, match=r"obs table, copy 1, column 7: source column \d+ is used twice"):
        hip.set_symmetry(types.SimpleNamespace(n_sym=2, obs=(perm, tab.obs[1]), critic=tab.critic, act=tab.act))
    perm[1, 7] = OD
    with pytest.raises(RlPpoError, match=r"obs table, copy 1, column 7: source column 45 outside 0..44"):
        hip.set_symmetry(types.SimpleNamespace(n_sym=2, obs=(perm, tab.obs[1]), critic=tab.critic, act=tab.act))
    sign = tab.act[1].copy()
    sign[1, 2] = 0.5
    with pytest.raises(RlPpoError, match=r"act table, copy 1, column 2: sign 0.5"):
        hip.set_symmetry(types.SimpleNamespace(n_sym=2, obs=tab.obs, critic=tab.critic, act=(tab.act[0], sign)))
    with pytest.raises(RlPpoError, match=r"critic table, copy 0, column \d+: copy 0 must be the identity"):
        hip.set_symmetry(types.SimpleNamespace(n_sym=1, obs=tab.obs, critic=(tab.critic[0][1:], tab.critic[1][1:]), act=tab.act))
    with pytest.raises(RlPpoError, match=r"n_sym 9 outside 1..8"):
        hip.set_symmetry(types.SimpleNamespace(n_sym=9, obs=tab.obs, critic=None, act=tab.act))
    assert hip.symmetry is None
    # late: after a mini-batch has run
    hip.minibatch_grad(_cast(st, torch.float32), _perm()[:37])
    with pytest.raises(RlPpoError, match="refused after the first rl_ppo_minibatch_grad / rl_ppo_update"):
        hip.set_symmetry(tab)
    hip.close()
    # twice
    hip = HipPPO(copy.deepcopy(pol).to(DEV), max_rows_per_minibatch=64, symmetry=tab)
    with pytest.raises(RlPpoError, match="already set"):
        hip.set_symmetry(tab)
    hip.close()
    with pytest.raises(ValueError, match="the table has 45 columns, the network's obs width is 44"):
        HipPPO(ActorCritic(OD - 1, CD, A).to(DEV), symmetry=tab)


def test_trainer_with_the_hip_learner_and_symmetry():
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv("RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0", num_envs=256, seed=42, device=DEV)
    tr = Trainer(env, seed=42, learner="hip", symmetry="lr")
    assert tr.symmetry.n_sym == 2 and tr.alg.symmetry is tr.symmetry and "symmetry=SymmetryTables(n_sym=2, obs=45, critic=48, act=12)" in repr(tr)
    for _ in range(3):
        out = tr.iterate()
        assert all(np.isfinite(out[k]) for k in ("value_loss", "surrogate_loss", "entropy", "kl", "learning_rate", "mean_reward", "action_std")), out
    sd = tr.state_dict()
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    pol = MlpPolicy.from_state_dict(sd, "actor", device=DEV)
    obs = torch.randn(256, pol.in_dim, device=DEV)
    torch.testing.assert_close(pol(obs).clone(), tr.actor(obs).clone(), rtol=0, atol=0)  # = the images the learner pushed
    torch.testing.assert_close(sd["std"].clamp_min(1e-6), tr.std, rtol=0, atol=0)
    pol.close()
    with pytest.raises(NotImplementedError, match="use_mirror_loss"):
        Trainer(env, learner="hip", symmetry="lr", use_mirror_loss=True)
    env.close()
