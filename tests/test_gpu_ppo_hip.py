"""`-m gpu`: the HIP PPO learner (include/rl_ppo.h, csrc/rl_ppo.hip, robot_lab_amd/ppo_hip.py) against the torch learner of
robot_lab_amd/ppo.py, which DEFINES the update rule.

The comparator everywhere is the unchanged `ppo.PPO` run in fp64 (`policy.double()`, storage cast to double) from the same initial
parameters with the same permutation; beside it the same `ppo.PPO` in fp32 on the same device measures what fp32 round-off alone does.
Nothing is compared against the code under test.  Bounds: the HIP learner and torch-fp32 are both fp32 evaluations of the same
expressions that differ in summation order only (an MFMA chain accumulates linearly over the contraction where a library GEMM may
tree-reduce), so a small multiple - 8 - of the fp32 learner's own distance from fp64 is legitimate; a missing term, a wrong ELU' mask
or bf16 products are 100 x or more.

Fixed synthetic inputs (no env): ActorCritic(45, 235, 12) under torch.manual_seed(0); a storage built by `fake_storage` of
tests/ppo_helpers.py with T = 24, N = 256 (6144 rows, mini-batches of 1536); then every parameter perturbed by 0.01 randn mean|p| so that
the probability ratio is not 1."""
import copy
import functools

import numpy as np
import pytest

from ppo_helpers import DEV, cast as _cast, fake_storage as _fake_storage, gen as _gen, perm as perm_of, split as _split, torch_learner as _torch_learner

pytestmark = pytest.mark.gpu

T, N, OD, CD, A = 24, 256, 45, 235, 12
B, MB = T * N, T * N // 4
_perm = functools.partial(perm_of, B)


@pytest.fixture(scope="module")
def case():
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pol = ActorCritic(OD, CD, A)
    st = _fake_storage(pol, T, N, OD, CD, A)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g) * p.abs().mean())
    return pol, st


@pytest.mark.parametrize("rows", [MB, 1000])
def test_gradient_parity_first_minibatch(case, rows):
    """e = max|g_hip - g64| / max|g64| <= 8 d, d = max|g32 - g64| / max|g64|, per parameter tensor (the table is profiles/ppo_hip_grad_parity.txt).
    The references' gradients come from `PPO.update` itself: one epoch of one mini-batch over exactly the rows of the first mini-batch
    (the loss is a mean over them, whatever their order) with a clipping norm so large that `clip_grad_norm_` multiplies by 1.
    rows = 1536: the first mini-batch of the update.  rows = 1000, on a handle created for 1536: the same check where the row count is
    no multiple of any tile - the row tails of the forward and dX tiles, a partial 16-row slice and empty chunks of the dW split, the tail
    of the loss head and of the column sums."""
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    idx = _perm()[:rows]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = _torch_learner(pol, dtype, num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30)
        alg.update(_cast(st, dtype, rows=idx), _gen(5))
        ref[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}
    hip = HipPPO(copy.deepcopy(pol).to(DEV), max_rows_per_minibatch=MB)
    g_hip = _split(hip.minibatch_grad(_cast(st, torch.float32), idx), pol)
    torch.cuda.synchronize()
    print(f"\n{rows} rows\n{'tensor':<18}{'max|g64|':>12}{'e (hip)':>12}{'d (torch32)':>13}{'e/d':>8}")
    bad = []
    for n, g64 in ref[torch.float64].items():
        scale = g64.abs().max().item()
        e = (g_hip[n].reshape(g64.shape) - g64).abs().max().item() / scale
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        print(f"{n:<18}{scale:12.4e}{e:12.3e}{d:13.3e}{e / d if d else float('inf'):8.2f}")
        if not e <= 8 * d:
            bad.append((n, e, d))
    assert not bad, f"gradient error above 8 x the fp32 torch learner's: {bad}"
    hip.close()


def test_one_update_matches_the_torch_learner(case):
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    a64, a32 = _torch_learner(pol, torch.float64), _torch_learner(pol, torch.float32)
    s64, s32 = a64.update(_cast(st, torch.float64), _gen()), a32.update(_cast(st, torch.float32), _gen())
    assert len(a64.lr_path) == 20 and a64.lr_path == a32.lr_path, "the two torch references took different learning-rate paths: the test is mis-built"
    hip = HipPPO(copy.deepcopy(pol).to(DEV))
    s_hip = hip.update(_cast(st, torch.float32), _gen())
    out = hip.store_into(copy.deepcopy(pol).to(DEV))
    torch.cuda.synchronize()
    p64 = {n: p.detach().double().cpu() for n, p in a64.policy.named_parameters()}
    p32 = {n: p.detach().double().cpu() for n, p in a32.policy.named_parameters()}
    ph = {n: p.detach().double().cpu() for n, p in out.named_parameters()}
    torch.testing.assert_close(_split(hip.flat("parameters"), pol)["std"], ph["std"], rtol=0, atol=0)  # store_into = the flat buffer
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
    assert abs(hip.last_grad_norm) > 0 and np.isfinite(hip.last_grad_norm)
    hip.close()


def test_update_is_deterministic(case):
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    st32, flats = _cast(st, torch.float32), []
    for _ in range(2):
        hip = HipPPO(copy.deepcopy(pol).to(DEV))
        hip.update(st32, _gen())
        flats.append(hip.flat("parameters").cpu())
        hip.close()
    assert torch.equal(flats[0], flats[1]) and bool(torch.isfinite(flats[0]).all())


def test_device_push_equals_host_set_weights(case, monkeypatch):
    """`rl_mlp_set_weights_device` writes three images per layer - the fp32 fragment image, the padded bias, the three bf16 planes - and each
    must equal what the host path (`rl_mlp_set_weights`) makes of the same numbers.  Every image is made to produce a compared output:
    the default forward reads the bf16 planes, the small-footprint launch (`rl_mlp_forward_small`, the 64-row case) and every forward under
    RL_MLP_PRECISION=f32 read the fp32 fragment image."""
    import torch

    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.ppo import mlp

    monkeypatch.delenv("RL_MLP_PRECISION", raising=False)
    torch.manual_seed(3)
    net0, net1 = mlp([OD, 512, 256, 128, A]).to(DEV), mlp([OD, 512, 256, 128, A]).to(DEV)
    lin = lambda m: [x for x in m if isinstance(x, torch.nn.Linear)]  # noqa: E731
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    a = MlpPolicy([host(x.weight) for x in lin(net0)], [host(x.bias) for x in lin(net0)], "elu", device=DEV)
    b = MlpPolicy([host(x.weight) for x in lin(net0)], [host(x.bias) for x in lin(net0)], "elu", device=DEV)
    X = [(x.weight.detach().contiguous(), x.bias.detach().contiguous()) for x in lin(net1)]
    a.set_weights_device([w for w, _ in X], [c for _, c in X])
    b.set_weights([w for w, _ in X], [c for _, c in X])

    def same(what, ya, yb, x):
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), f"{what}: device push and host set_weights give different outputs"
        torch.testing.assert_close(ya, net1(x).detach(), rtol=2e-5, atol=2e-5)  # ... and they are the new network's

    x4096, x64 = torch.randn(4096, OD, device=DEV), torch.randn(64, OD, device=DEV)
    for x in (x4096, x64):  # default precision: the bf16 planes and the bias
        same(f"{x.shape[0]} rows, split-bf16 forward", a(x).clone(), b(x).clone(), x)
    ya, yb = torch.zeros(64, A, device=DEV), torch.ones(64, A, device=DEV)  # the small-batch kernel: the fp32 fragment image
    a.forward_into(x64, ya.data_ptr(), small=True)
    b.forward_into(x64, yb.data_ptr(), small=True)
    same("64 rows, small-footprint kernel", ya, yb, x64)
    monkeypatch.setenv("RL_MLP_PRECISION", "f32")  # (read by the library at every call)
    for x in (x4096, x64):
        same(f"{x.shape[0]} rows, exact-f32 forward", a(x).clone(), b(x).clone(), x)
    a.close(); b.close()


@pytest.mark.parametrize("branch", ["fall", "hold", "rise"])
def test_schedule_branches_follow_the_torch_learner(case, branch):
    """desired_kl chosen from the fp64 reference's KL of the first mini-batch, a factor 2 away from either threshold of its branch; one epoch
    of four mini-batches, the HIP learner stepped one mini-batch at a time so that its learning-rate word can be read after each."""
    import torch

    from robot_lab_amd.ppo import gaussian_kl
    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    perm = _perm()
    idx = perm[:MB]
    p64, st64 = copy.deepcopy(pol).to(device=DEV, dtype=torch.float64), _cast(st, torch.float64)
    with torch.no_grad():
        mean, std = p64.distribution(st64.observations.reshape(B, OD)[idx])
        kl = float(gaussian_kl(st64.mu.reshape(B, A)[idx], st64.sigma.reshape(B, A)[idx], mean, std).mean())
    assert kl > 0
    desired = {"fall": kl / 4.0, "hold": kl, "rise": 4.0 * kl}[branch]  # thresholds 2 desired and desired / 2
    kw = dict(num_learning_epochs=1, num_mini_batches=4, desired_kl=desired, learning_rate=1e-3)
    ref = _torch_learner(pol, torch.float32, **kw)
    ref.update(_cast(st, torch.float32), _gen())
    first = {"fall": 1e-3 / 1.5, "hold": 1e-3, "rise": 1.5e-3}[branch]
    assert ref.lr_path[0] == first, "the torch learner did not take the intended branch: the test is mis-built"
    hip = HipPPO(copy.deepcopy(pol).to(DEV), **dict(kw, num_mini_batches=1))
    st32, path = _cast(st, torch.float32), []
    for i in range(4):
        path.append(hip.update(st32, perm=perm[i * MB:(i + 1) * MB])["learning_rate"])
    print(f"\n[{branch}] kl64 {kl:.5f} desired {desired:.5f} lr path hip {path} torch {ref.lr_path}")
    assert path == ref.lr_path
    hip.close()


def test_fixed_schedule_keeps_the_learning_rate(case):
    import torch

    from robot_lab_amd.ppo_hip import HipPPO

    pol, st = case
    hip = HipPPO(copy.deepcopy(pol).to(DEV), schedule="fixed", learning_rate=3e-4, num_learning_epochs=1)
    out = hip.update(_cast(st, torch.float32), _gen())
    assert out["learning_rate"] == 3e-4 and out["kl"] == 0.0 and np.isfinite(out["value_loss"])
    hip.close()


def test_a1_learns_to_track_velocity_commands_with_the_hip_learner():
    """tests/test_gpu_train.py::test_a1_learns_to_track_velocity_commands with `learner="hip"`"""
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.ppo import Trainer

    N, iters = 2048, 60
    env = ManagerBasedRLEnv("RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0", num_envs=N, seed=42, device="cuda:0")
    tr = Trainer(env, seed=42, learner="hip")
    assert tr.learner == "hip" and "HipPPO" in repr(tr) and type(tr.alg).__name__ == "HipPPO"
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (N,), generator=torch.Generator().manual_seed(0))
    rew, err, done = [], [], []
    for it in range(iters):
        out = tr.iterate()
        rew.append(out["mean_reward"])
        done.append(out["done_rate"])
        ex = env.extras.get("log", {})
        if "Metrics/base_velocity/error_vel_xy" in ex:
            err.append(float(ex["Metrics/base_velocity/error_vel_xy"]))
        assert np.isfinite(out["value_loss"]) and np.isfinite(out["surrogate_loss"])
    first, last = float(np.mean(rew[:5])), float(np.mean(rew[-5:]))
    print(f"\n[train, HIP learner] A1 Flat {N} envs: reward/step {first:+.4f} -> {last:+.4f}; done/step {np.mean(done[:5]):.4f} -> {np.mean(done[-5:]):.4f}; "
          f"std {out['action_std']:.3f}; lr {out['learning_rate']:.1e}")
    assert last > first + 0.5 * abs(first) or last > first + 0.01, "the mean step reward did not improve in 60 PPO iterations"
    assert np.mean(done[-5:]) <= np.mean(done[:5]) + 1e-3, "episodes end more often than at the start: the policy is falling over more"
    sd = tr.state_dict()
    assert {"std", "actor.0.weight", "actor.6.bias", "critic.6.weight"} <= set(sd)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    pol = MlpPolicy.from_state_dict(sd, "actor", device="cuda:0")  # the checkpoint layout the inference side reads
    obs = torch.randn(256, pol.in_dim, device="cuda:0")
    torch.testing.assert_close(pol(obs).clone(), tr.actor(obs).clone(), rtol=0, atol=0)  # = the images the learner pushed
    torch.testing.assert_close(sd["std"].clamp_min(1e-6), tr.std, rtol=0, atol=0)
    pol.close()
    env.close()
