"""`-m gpu`: `Trainer(..., normalize_in_learner=True)` end to end - observation normalisation together with symmetry, either learner reading the RAW
storage (robot_lab_amd/ppo.py, ppo_hip.py; the kernels: the NORM side of csrc/rl_ppo.hip).  A1 Flat, 64 envs, T = 8.  The comparator is the
rule of robot_lab_amd.ppo (`PPO(symmetry=...)` through the normaliser modules on raw rows, pinned by tests/test_ppo_obsnorm_symmetry.py) in
fp64, fp32 beside it for the yardstick; the bounds are those of tests/test_gpu_obsnorm_train.py::test_both_learners_on_the_same_collected_batch."""
import copy
import types

import numpy as np
import pytest

from ppo_helpers import DEV, cast as _cast, gen as _gen, perm as perm_of, split as _split, torch_learner as _torch_learner

pytestmark = pytest.mark.gpu
A1 = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
T, N = 8, 64
B, MB = T * N, T * N // 4
BUFFERS = ("observations", "privileged_observations", "actions", "mu", "sigma", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages")
BOTH = dict(actor_obs_normalization=True, critic_obs_normalization=True)


def _trainer(n=N, seed=3, steps=T, **kw):
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1, num_envs=n, seed=seed, device=DEV)
    return Trainer(env, num_steps_per_env=steps, seed=seed, **kw)


def _close(*trainers):
    for tr in trainers:
        tr.env.close()


def _bits(st):
    import torch

    return {k: getattr(st, k).clone().view(torch.uint8 if k == "dones" else torch.int32) for k in BUFFERS}


def test_both_learners_on_the_same_collected_batch_with_symmetry():
    """`Trainer(symmetry="lr", both flags, normalize_in_learner=True)`: the HIP learner normalises the mirrored raw rows in its fetch, the torch
    learner through the modules' forward.  Gradient of the first mini-batch: e <= 8 d per tensor (no floor); parameters after one
    update (fixed schedule, 20 steps on 128-row mini-batches x 2 copies): q999 <= max(8 q999 of torch-fp32, one spacing), max <= the
    displacement Adam allows.  The torch learner inside its Trainer IS the rule in fp32: bit for bit the fp32 comparator."""
    import torch

    kw = dict(symmetry="lr", schedule="fixed", normalize_in_learner=True, **BOTH)
    tr, tt = _trainer(learner="hip", **kw), _trainer(learner="torch", **kw)
    assert "normalize_in_learner=True" in repr(tr) and "obs_normalizers=['actor', 'critic']" in repr(tr.alg) and tr.symmetry.n_sym == 2
    for t in (tr, tt):
        t.collector.collect()
        assert t.update_batch() is t.storage, "normalize_in_learner: the learner reads the raw storage, no scratch matrices"
    a, b = _bits(tr.storage), _bits(tt.storage)
    for k in BUFFERS:
        assert torch.equal(a[k], b[k]), k  # (same seed, same parameters: the same batch)
    torch.cuda.synchronize()
    pol = copy.deepcopy(tr.policy).cpu()
    assert int(pol.actor_obs_normalizer.count) == int(pol.critic_obs_normalizer.count) == T * N and float(pol.actor_obs_normalizer._mean.abs().max()) > 0
    raw = types.SimpleNamespace(num_transitions_per_env=T, num_envs=N, **{k: getattr(tr.storage, k).clone() for k in BUFFERS if k != "dones"})
    idx = perm_of(B)[:MB]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = _torch_learner(pol, dtype, symmetry=tr.symmetry, num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30, schedule="fixed")
        alg.update(_cast(raw, dtype, rows=idx), _gen(5))
        ref[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}
    g_hip = _split(tr.alg.minibatch_grad(tr.storage, idx), pol)
    bad = []
    print(f"\nA1 Flat 64 x 8, symmetry lr, both groups normalised in the learner\n{'tensor':<18}{'max|g64|':>12}{'e (hip)':>12}{'d (torch32)':>13}{'e/d':>8}")
    for n, g64 in ref[torch.float64].items():
        scale = g64.abs().max().item()
        e = (g_hip[n].reshape(g64.shape) - g64).abs().max().item() / scale
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        print(f"{n:<18}{scale:12.4e}{e:12.3e}{d:13.3e}{e / d if d else float('inf'):8.2f}")
        if not e <= 8 * d:
            bad.append((n, e, d))
    assert not bad, f"gradient error above 8 x the fp32 torch learner's: {bad}"
    a64, a32 = (_torch_learner(pol, dtype, symmetry=tr.symmetry, schedule="fixed") for dtype in (torch.float64, torch.float32))
    a64.update(_cast(raw, torch.float64), _gen())
    a32.update(_cast(raw, torch.float32), _gen())
    tr.alg.update(tr.update_batch(), _gen())
    tt.alg.update(tt.update_batch(), _gen())
    out = tr.alg.store_into(copy.deepcopy(tr.policy))
    torch.cuda.synchronize()
    displacement = float(sum(a64.lr_path))
    assert len(a64.lr_path) == 20
    bad = []
    print(f"\n{'tensor':<18}{'q999 hip':>12}{'q999 torch32':>14}{'max hip':>12}{'max torch32':>13}")
    for (n, p64), (_, p32), (_, ph), (_, pt) in zip(a64.policy.named_parameters(), a32.policy.named_parameters(), out.named_parameters(), tt.policy.named_parameters()):
        assert torch.equal(pt.detach(), p32.detach()), f"{n}: the torch learner in the Trainer is not the fp32 rule on the raw rows"
        p64, p32, ph = (p.detach().double().cpu() for p in (p64, p32, ph))
        dh, d32 = (ph - p64).abs().flatten(), (p32 - p64).abs().flatten()
        qh, q32 = torch.quantile(dh, 0.999).item(), torch.quantile(d32, 0.999).item()
        ulp = float(np.spacing(np.float32(p64.abs().max().item())))
        print(f"{n:<18}{qh:12.3e}{q32:14.3e}{dh.max().item():12.3e}{d32.max().item():13.3e}")
        if not qh <= max(8 * q32, ulp):
            bad.append((n, "q999", qh, q32))
        if not dh.max().item() <= displacement:
            bad.append((n, "max", dh.max().item(), displacement))
    assert not bad, bad
    _close(tr, tt)


def test_scratch_and_learner_paths_agree_bit_for_bit_without_symmetry():
    """`normalize_in_learner` True / False on the same seed: the collection is untouched (the same storage bits), and the HIP learner's update from
    the raw rows leaves the parameters and Adam moments of the update from the scratch matrices - every bit"""
    import torch

    from robot_lab_amd.ppo import NormalizedBatch

    fused, scratch = _trainer(learner="hip", normalize_in_learner=True, **BOTH), _trainer(learner="hip", **BOTH)
    assert isinstance(scratch._batch, NormalizedBatch) and fused._batch is fused.storage and "normalize_in_learner" not in repr(scratch)
    for it in range(2):
        for tr in (fused, scratch):
            tr.collector.collect()
        a, b = _bits(fused.storage), _bits(scratch.storage)
        for k in BUFFERS:
            assert torch.equal(a[k], b[k]), f"iteration {it}: {k} differs in {int((a[k] != b[k]).sum())} entries"
        stats = [tr.alg.update(tr.update_batch(), tr.gen) for tr in (fused, scratch)]
        assert stats[0] == stats[1], stats
        for w in ("parameters", "exp_avg", "exp_avg_sq"):
            assert torch.equal(fused.alg.flat(w), scratch.alg.flat(w)), f"iteration {it}: {w}"
        for tr in (fused, scratch):
            tr._push_weights()
    _close(fused, scratch)


@pytest.mark.parametrize("src,dst", [("hip", "torch"), ("torch", "hip")])
def test_a_checkpoint_crosses_the_learners(src, dst):
    import torch

    kw = dict(symmetry="lr", normalize_in_learner=True, **BOTH)
    one, two = _trainer(learner=src, **kw), _trainer(learner=dst, seed=4, **kw)
    for _ in range(2):
        one.iterate()
    sd = {k: v.clone() for k, v in one.state_dict().items()}
    assert int(sd["actor_obs_normalizer.count"]) == int(sd["critic_obs_normalizer.count"]) == 2 * T * N
    two.policy.load_state_dict(sd)
    if dst == "hip":
        two.alg.load_from(two.policy)
    two.push_parameters()
    for h1, h2 in zip(one.normalizers, two.normalizers):
        for x, y in zip(h1.get_state()[:3], h2.get_state()[:3]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert h1.get_state()[3] == h2.get_state()[3] == 2 * T * N
    back = two.state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    obs = one.collector.obs["policy"].clone()
    assert torch.equal(one.actor(one.normalizers[0].apply(obs)).clone(), two.actor(two.normalizers[0].apply(obs)).clone())
    out = two.iterate()  # the resumed training runs, through the other learner
    assert all(np.isfinite(out[k]) for k in ("value_loss", "surrogate_loss", "entropy", "kl", "learning_rate")), out
    assert two.normalizers[0].get_state()[3] == 3 * T * N
    _close(one, two)


def test_refusals():
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1, num_envs=N, seed=3, device=DEV)
    with pytest.raises(NotImplementedError, match="symmetry") as e:  # the default call: unchanged, and the message names the way out
        Trainer(env, num_steps_per_env=T, symmetry="lr", actor_obs_normalization=True)
    assert "normalize_in_learner=True" in str(e.value)
    for learner in ("torch", "hip"):
        with pytest.raises(ValueError, match="normalize_in_learner=True without actor_obs_normalization / critic_obs_normalization"):
            Trainer(env, num_steps_per_env=T, learner=learner, normalize_in_learner=True)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        Trainer(env, num_steps_per_env=T, critic_obs_normalization=True, normalize_in_learner=True, group=types.SimpleNamespace(world_size=2, enabled=True))
    env.close()


def test_a_short_run_with_symmetry_and_normalisation_in_the_hip_learner():
    """Ten iterations of A1 Flat (512 envs) with `symmetry="lr"`, the mirror loss, both groups normalised in the HIP learner's fetch: every statistic
    finite, the critic learns (the value loss falls: mean of the last three iterations below the mean of the first three).  The 60-iteration
    criterion of tests/test_gpu_obsnorm_train.py::test_a1_learns_to_track_velocity_commands_with_normalisation is NOT kept as a test: with
    `symmetry="lr"` on top it is met (reward per step -0.0009 -> +0.0029, done rate unchanged), but it takes 3.1 s where that test takes 1.3 s in
    the same session - two copies per row in every update - so this is the ten-iteration form."""
    import torch

    n, iters = 512, 10
    tr = _trainer(n=n, seed=42, steps=24, learner="hip", symmetry="lr", mirror_loss=0.5, normalize_in_learner=True, **BOTH)
    tr.env.episode_length_buf = torch.randint(0, tr.env.max_episode_length, (n,), generator=torch.Generator().manual_seed(0))
    vloss = []
    for _ in range(iters):
        out = tr.iterate()
        assert all(np.isfinite(out[k]) for k in ("value_loss", "surrogate_loss", "entropy", "kl", "mirror_loss", "learning_rate", "mean_reward", "action_std")), out
        vloss.append(out["value_loss"])
    print(f"\n[train, symmetry + normalisation in the learner] value loss {['%.4f' % v for v in vloss]}")
    assert np.mean(vloss[-3:]) < np.mean(vloss[:3]), vloss
    sd = tr.state_dict()
    assert int(sd["actor_obs_normalizer.count"]) == iters * 24 * n and all(bool(torch.isfinite(v).all()) for v in sd.values())
    _close(tr)
