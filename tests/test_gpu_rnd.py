"""`-m gpu`: random network distillation on the device (include/rl_rnd.h, include/rl_rnd_learner.h, robot_lab_amd/rnd_hip.py, collect.py, ppo.py).

Exact families have no tolerance.  Bounded families use the project's bound (tests/rnd_helpers.py `bound_ratio`): e <= 8 d, e the device's and d the
fp32 reference's own distance from the fp64 rule, both relative to max|ref64|.  With RND_PARITY_OUT=<file> in the environment the measured
ratios e / d are written there (profiles/rnd_parity.txt)."""
import copy
import os
import types

import numpy as np
import pytest

from ppo_helpers import DEV, fake_storage
from rnd_helpers import NpRnd, bound_ratio, cast_layers, make_layers, module_from_layers, module_tensors

pytestmark = pytest.mark.gpu
A1F = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
T, N = 4, 64
BUFFERS = ("observations", "privileged_observations", "actions", "mu", "sigma", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages")
LINES = []


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    out = os.environ.get("RND_PARITY_OUT")
    if out and LINES:
        with open(out, "w") as f:
            f.write("RND on the device against the rule (robot_lab_amd/rnd.py) in fp64; d: the fp32 reference's own distance; the bound is e <= 8 d\n"
                    f"{'case':<52}{'quantity':<26}{'e (hip)':>12}{'d (fp32)':>12}{'e/d':>8}\n" + "\n".join(LINES) + "\n")


def _bound(title, name, got, r64, r32, bad):
    e, d, ratio = bound_ratio(got, r64, r32)
    line = f"{title:<52}{name:<26}{e:12.3e}{d:12.3e}{(e / d if d else float('inf')):8.2f}"
    print(line)
    LINES.append(line)
    if not ratio <= 1.0:
        bad.append((title, name, e, d))


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


# ---- exact, no tolerance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 512])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_row_norm_the_weight_and_the_addition_are_exact(n, K):
    """Integer embeddings whose difference is (3 2^k, 0, .., 0, 4 2^k) - the first and the last column: both ends of the reduction - give 5 2^k;
    K = 1 gives |d|.  Weight 2^j; the reward slot holds integers and its neighbours stay untouched."""
    import torch

    from robot_lab_amd.rnd_hip import RndReward

    rng = np.random.default_rng(100 * n + K)
    k = rng.integers(0, 7, n)
    pred = rng.integers(-64, 65, (n, K)).astype(np.float32)
    diff = np.zeros((n, K), np.float32)
    if K == 1:
        diff[:, 0] = rng.choice([-1.0, 1.0], n) * rng.integers(0, 9, n) * 2.0 ** k
        want = np.abs(diff[:, 0])
    else:
        sign = rng.choice([-1.0, 1.0], (n, 2))
        diff[:, 0], diff[:, -1] = sign[:, 0] * 3 * 2.0 ** k, sign[:, 1] * 4 * 2.0 ** k
        want = 5 * 2.0 ** k
    targ = pred + diff
    weights = [0.5, 4.0, 1.0]
    slots = rng.integers(-100, 101, (5, n)).astype(np.float32)
    for arr in (targ, want, slots[2] + 4.0 * want):
        assert np.array_equal(arr.astype(np.float32).astype(np.float64), arr.astype(np.float64))  # exact in fp32
    h = RndReward(n, K, 3, gamma=0.5, device=DEV)
    h.set_weights(weights)
    buf = _dev(slots)
    h.step(_dev(pred), _dev(targ), 1, buf[2])
    torch.cuda.synchronize()
    assert np.array_equal(h.r.cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(h.avg.cpu().numpy(), want.astype(np.float32))
    got = buf.cpu().numpy()
    assert np.array_equal(got[2], slots[2] + 4.0 * want.astype(np.float32))
    assert np.array_equal(got[[0, 1, 3, 4]], slots[[0, 1, 3, 4]])
    intrinsic, total = h.sums(2)  # steps 0 and 1; step 0 never ran: its partials are the zeros of creation
    assert intrinsic == float((4.0 * want).sum()) and total == float((slots[2] + 4.0 * want).sum())
    # the two-launch route gives the same bits, and divides by the std word
    buf2, std = _dev(slots), _dev([[2.0]])
    h.rows(_dev(pred), _dev(targ))
    h.finish(1, buf2[2], std)
    torch.cuda.synchronize()
    assert np.array_equal(buf2.cpu().numpy()[2], slots[2] + 2.0 * want.astype(np.float32))
    assert np.array_equal(h.avg.cpu().numpy(), (1.5 * want).astype(np.float32))  # avg 0.5 + r
    h.finish(0, buf2[0], _dev([[0.0]]))  # std == 0: the reward is not divided
    torch.cuda.synchronize()
    assert np.array_equal(buf2.cpu().numpy()[0], slots[0] + 0.5 * want.astype(np.float32))
    h.close()


def test_the_discounted_average_is_the_fp64_recursion():
    import torch

    from robot_lab_amd.rnd_hip import RndReward

    n = 65
    rng = np.random.default_rng(5)
    rewards = rng.integers(0, 33, (4, n)).astype(np.float64)
    want, avg = [], np.zeros(n)
    for t in range(4):
        avg = avg * 0.5 + rewards[t]
        want.append(avg.copy())
    for a in want:  # exact in fp32 before anything runs: integers / 8 below 2^24
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    h = RndReward(n, 1, 4, gamma=0.5, device=DEV)
    zero = torch.zeros(n, 1, device=DEV)
    for t in range(4):
        h.rows(zero, _dev(rewards[t].reshape(n, 1)))
        torch.cuda.synchronize()
        assert np.array_equal(h.avg.cpu().numpy().astype(np.float64), want[t]), t
    h.reset()
    torch.cuda.synchronize()
    assert not h.avg.any()
    h.close()


def _trainer(seed=3, n=N, **kw):
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1F, num_envs=n, seed=seed, device=DEV)
    return Trainer(env, num_steps_per_env=T, seed=seed, **kw)


def _close(*trainers):
    for tr in trainers:
        tr.env.close()


def _storage_bits(st):
    import torch

    return {k: getattr(st, k).clone().view(torch.uint8 if k == "dones" else torch.int32) for k in BUFFERS}


def _assert_same_storage(a, b, what):
    import torch

    for k in BUFFERS:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} entries"


RND = dict(weight=0.5, predictor_hidden_dims=[64, 32], target_hidden_dims=[48], num_outputs=4)
RND_FULL = dict(RND, reward_normalization=True, state_normalization=True, weight_schedule=dict(mode="linear", initial_step=2, final_step=11, final_value=0.05))


def test_weight_zero_collects_the_storage_of_a_trainer_without_rnd():
    off, on = _trainer(), _trainer(rnd=dict(RND, weight=0.0))
    assert off.rnd is None and off.collector.rnd is None and "rnd" not in repr(off) and on.collector.rnd is on.rnd_device
    for it in range(2):
        for tr in (off, on):
            tr.collector.collect()
        _assert_same_storage(_storage_bits(off.storage), _storage_bits(on.storage), f"iteration {it}")
    assert float(on.rnd_device.reward.r.abs().max()) > 0  # the launches ran
    _close(off, on)


# ---- bounded -----------------------------------------------------------------------------------------------------------------------------
def _reward_case(S, K=4, n=257, seed=0, converged=False):
    rng = np.random.default_rng(seed + S)
    targ = make_layers(rng, [S, 48, K])
    if converged:
        pred = [(w + 1e-3 * rng.standard_normal(w.shape), b + 1e-3 * rng.standard_normal(b.shape)) for w, b in targ]
    else:
        pred = make_layers(rng, [S, 64, 32, K])
    states = rng.standard_normal((T, n, S)) * np.linspace(0.5, 2.0, S) + 0.3
    slots = rng.standard_normal((T, n))
    return cast_layers(pred, np.float32), cast_layers(targ, np.float32), states.astype(np.float32), slots.astype(np.float32)


def _device_rewards(pred, targ, states, slots, **kw):
    import torch

    from robot_lab_amd.rnd_hip import RndDevice

    m = module_from_layers(pred, targ, torch.float32, **kw).to(DEV)
    dev = RndDevice(m, states.shape[1], T, device=DEV)
    buf, xs = _dev(slots), _dev(states)
    dev.begin_iteration()
    out = []
    for t in range(T):
        dev.step(t, xs[t], buf[t])
        out.append((buf[t] - _dev(slots[t])).cpu().numpy())
    torch.cuda.synchronize()
    res = np.stack(out), buf.cpu().numpy(), dev.reward.sums()
    dev.close()
    return res


@pytest.mark.parametrize("S", [45, 235, 512])
def test_the_intrinsic_reward_is_within_the_bound_of_the_fp64_rule(S):
    """both normalisers on, a step schedule inside the window; ref64 / ref32: the torch rule on the host in fp64 / fp32"""
    import torch

    pred, targ, states, slots = _reward_case(S)
    kw = dict(weight=0.7, weight_schedule=dict(mode="step", final_step=3, final_value=0.25), state_normalization=True, reward_normalization=True)
    _, total, sums = _device_rewards(pred, targ, states, slots, **kw)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = module_from_layers(pred, targ, dtype, **kw)
        buf = torch.as_tensor(slots).to(dtype).clone()
        r = torch.stack([m.collect_step(buf[t], torch.as_tensor(states[t]).to(dtype)) for t in range(T)])
        ref[dtype] = (r.numpy(), buf.numpy())
    bad = []
    got_r = total.astype(np.float64) - slots  # (the slot's own rounding is part of what is measured: compared on the sums below)
    _bound(f"reward S={S} both normalisers", "slot after the addition", total, ref[torch.float64][1], ref[torch.float32][1], bad)
    assert not bad, bad
    assert np.abs(got_r - ref[torch.float64][0]).max() <= 2.0 ** -22 * np.abs(total).max() + 8 * max(np.abs(ref[torch.float32][0] - ref[torch.float64][0]).max(), 1e-7)
    assert sums[1] == pytest.approx(float(total.astype(np.float64).sum()), rel=1e-12)
    assert sums[0] == pytest.approx(float(ref[torch.float64][0].sum()), rel=1e-4)


def test_a_nearly_converged_predictor_is_within_the_bound_of_the_numpy_fp32_emulation():
    """target + a 1e-3 perturbation: the difference cancels, so what is left is the networks' own fp32 round-off.  No normalisers: r itself."""
    pred, targ, states, slots = _reward_case(45, converged=True)
    zeros = np.zeros_like(slots)
    r_dev, _, _ = _device_rewards(pred, targ, states, zeros, weight=1.0)
    ref = {}
    for dtype in (np.float64, np.float32):
        rule = NpRnd(cast_layers(pred, dtype), cast_layers(targ, dtype), weight=1.0)
        buf = zeros.astype(dtype).copy()
        ref[dtype] = np.stack([rule.collect_step(buf[t], states[t]) for t in range(T)])
    assert float(ref[np.float64].max()) < 0.1  # it cancels
    bad = []
    _bound("reward S=45 converged predictor", "r_int", r_dev, ref[np.float64], ref[np.float32], bad)
    assert not bad, bad


def _update_case(seed=2, S=45, K=4, rows=256):
    rng = np.random.default_rng(seed)
    pred, targ = make_layers(rng, [S, 64, 32, K]), make_layers(rng, [S, 64, 32, K])
    state = rng.standard_normal((rows, S)) * np.linspace(0.5, 2.0, S) + 0.3
    return cast_layers(pred, np.float32), cast_layers(targ, np.float32), state.astype(np.float32), rng.permutation(rows)


def _hip_learner(pred, targ, state, **kw):
    import torch

    from robot_lab_amd.obsnorm import ObsNormalizer
    from robot_lab_amd.rnd_hip import HipRND

    m = module_from_layers(pred, targ, torch.float32, weight=1.0, state_normalization=True, **kw)
    m.state_normalizer.update(torch.as_tensor(state))
    m = m.to(DEV)
    h = ObsNormalizer(state.shape[1], m.state_normalizer.eps, max_rows=state.shape[0], device=DEV)
    h.load_module(m.state_normalizer)
    return m, h, HipRND(m, num_learning_epochs=2, num_mini_batches=2, max_rows_per_minibatch=state.shape[0] // 2, state_normalizer=h)


def _torch_update(pred, targ, state, perm, dtype, grad_only=False):
    import torch

    from robot_lab_amd.rnd import make_optimizer, update_minibatch

    m = module_from_layers(pred, targ, dtype, weight=1.0, state_normalization=True)
    m.state_normalizer.update(torch.as_tensor(state).to(dtype))
    rows, opt = torch.as_tensor(state).to(dtype), make_optimizer(m)
    mb = len(perm) // 2
    if grad_only:
        m.loss(rows[torch.as_tensor(perm[:mb])]).backward()
        return {f"grad.{n}": p.grad.double().numpy() for n, p in m.predictor.named_parameters()}
    losses = [update_minibatch(m, opt, rows[torch.as_tensor(perm[i * mb:(i + 1) * mb])]) for _ in range(2) for i in range(2)]
    return module_tensors(m, opt), float(np.mean(losses))


def _split(flat, module, prefix):
    out, o = {}, 0
    flat = flat.detach().cpu().double().numpy()
    for n, p in module.predictor.named_parameters():
        out[f"{prefix}.{n}"] = flat[o:o + p.numel()].reshape(tuple(p.shape))
        o += p.numel()
    assert o == flat.size
    return out


def test_one_whole_update_is_within_the_bound_of_the_fp64_rule():
    """2 x 2 mini-batches over 256 rows, hidden 64-32, state normalisation through the scratch pass: the predictor's gradient of the first
    mini-batch, every tensor; then parameters and Adam moments after the update; the target bit for bit; two runs bit for bit."""
    import torch

    pred, targ, state, perm = _update_case()
    perm_t = torch.as_tensor(perm).to(DEV)
    runs = []
    for _ in range(2):
        m, h, alg = _hip_learner(pred, targ, state)
        grad = _split(alg.minibatch_grad(_dev(state), perm_t[:128]), m, "grad")
        alg.update(_dev(state), perm_t)
        stats = alg.stats()
        assert alg.adam_step == 4
        got = {**_split(alg.flat("parameters"), m, "predictor"), **_split(alg.flat("exp_avg"), m, "exp_avg"), **_split(alg.flat("exp_avg_sq"), m, "exp_avg_sq")}
        ws, bs = alg.target_parameters()
        torch.cuda.synchronize()
        for l, (w, b) in enumerate(targ):  # never written
            assert np.array_equal(ws[l].cpu().numpy().view(np.int32), w.view(np.int32)) and np.array_equal(bs[l].cpu().numpy().view(np.int32), b.view(np.int32))
        stored = alg.store_into(copy.deepcopy(m))
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in stored.predictor.parameters()]), alg.flat("parameters"))
        runs.append((grad, got, stats))
        alg.close()
        h.close()
    for a, b in zip(runs[0][:2], runs[1][:2]):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert runs[0][2] == runs[1][2]
    grad, got, stats = runs[0]
    g64, g32 = (_torch_update(pred, targ, state, perm, d, grad_only=True) for d in (torch.float64, torch.float32))
    (t64, l64), (t32, l32) = (_torch_update(pred, targ, state, perm, d) for d in (torch.float64, torch.float32))
    bad = []
    for name in g64:
        _bound("update 256 rows 64-32, first mini-batch", name, grad[name], g64[name], g32[name], bad)
    for name in got:
        _bound("update 256 rows 64-32, after 2 x 2 mini-batches", name, got[name], t64[name], t32[name], bad)
    assert not bad, bad
    assert abs(stats["rnd_loss"] - l64) <= 8 * max(abs(l32 - l64), float(np.spacing(np.float32(l64))))


# ---- structure ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_the_eager_loop_bit_for_bit():
    import torch

    eager, graph = _trainer(use_graph=False, rnd=RND_FULL), _trainer(use_graph=True, rnd=RND_FULL)
    for it in range(3):  # the graph trainer: eager once, captured and replayed, replayed; the linear schedule moves the weight in every step
        for tr in (eager, graph):
            tr.collector.collect()
        _assert_same_storage(_storage_bits(eager.storage), _storage_bits(graph.storage), f"iteration {it}")
        for name in ("r", "avg", "weights"):
            a, b = getattr(eager.rnd_device.reward, name), getattr(graph.rnd_device.reward, name)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (it, name)
        for which in ("state_norm", "reward_norm"):
            for a, b in zip(getattr(eager.rnd_device, which).get_state(), getattr(graph.rnd_device, which).get_state()):
                assert a == b if isinstance(a, int) else torch.equal(a.view(torch.int32), b.view(torch.int32)), (it, which)
        assert eager.rnd_device.reward.sums() == graph.rnd_device.reward.sums()
    assert graph.collector._graph is not None and eager.collector._graph is None
    assert eager.rnd.update_counter == 3 * T and eager.rnd_device.state_norm.get_state()[3] == 3 * T * N
    _close(eager, graph)


@pytest.mark.parametrize("group", ["policy", "critic"])
def test_the_added_reward_is_the_fp64_replay_of_the_rule_on_the_stored_observations(group):
    """rewards_on - rewards_off against the rule in fp64 (numpy) on what the storage holds: the new observation of step t is slot t + 1, the one of
    the last step is what collect() returns - post-reset rows where an env was done.  Bound: the slot's own rounding (half a spacing of the largest
    |reward|, twice: the sum and the difference) + 8 x the fp32 rule's own distance from fp64."""
    import torch

    rnd = dict(RND_FULL, group=group)
    off, on = _trainer(), _trainer(use_graph=False, rnd=rnd)
    on.env.episode_length_buf = on.env.max_episode_length - 1 - (torch.arange(N) % 6)  # time-outs inside the window: resets and bootstraps
    off.env.episode_length_buf = off.env.max_episode_length - 1 - (torch.arange(N) % 6)
    lin = lambda seq: [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in seq if isinstance(m, torch.nn.Linear)]  # noqa: E731
    pred, targ = lin(on.rnd.predictor), lin(on.rnd.target)
    last_off, last_on = off.collector.collect(), on.collector.collect()
    torch.cuda.synchronize()
    key = "observations" if group == "policy" else "privileged_observations"
    stored = getattr(on.storage, key).cpu().numpy()
    assert np.array_equal(stored, getattr(off.storage, key).cpu().numpy()) and bool(on.storage.dones.any())
    new = [stored[t + 1] for t in range(T - 1)] + [last_on[group].cpu().numpy()]
    base, total = off.storage.rewards.cpu().numpy(), on.storage.rewards.cpu().numpy()
    ref = {}
    for dtype in (np.float64, np.float32):
        rule = NpRnd(cast_layers(pred, dtype), cast_layers(targ, dtype), weight=rnd["weight"], schedule=rnd["weight_schedule"], state_normalization=True,
                     reward_normalization=True)
        buf = base.astype(dtype).copy()
        ref[dtype] = np.stack([rule.collect_step(buf[t], new[t]) for t in range(T)])
    diff = total.astype(np.float64) - base
    tol = 2.0 ** -23 * np.abs(total).max() + 8 * np.abs(ref[np.float32].astype(np.float64) - ref[np.float64]).max()
    worst = np.abs(diff - ref[np.float64]).max()
    print(f"group {group}: max|added - fp64 rule| {worst:.3e}, allowed {tol:.3e}, max r_int {ref[np.float64].max():.3e}")
    assert float(ref[np.float64].min()) > 0 and worst <= tol
    intrinsic, summed = on.rnd_device.reward.sums()
    assert summed == pytest.approx(float(total.astype(np.float64).sum()), rel=1e-12) and intrinsic == pytest.approx(float(ref[np.float64].sum()), rel=1e-4)
    _close(off, on)


def test_the_ppo_half_of_the_hip_update_does_not_notice_rnd():
    import torch

    from robot_lab_amd.ppo import ActorCritic
    from robot_lab_amd.ppo_hip import HipPPO
    from robot_lab_amd.rnd_hip import HipRND

    torch.manual_seed(0)
    pol = ActorCritic(10, 14, 3, actor_hidden=(32, 16), critic_hidden=(32, 16))
    st = fake_storage(pol, T=4, N=64)
    dev_st = types.SimpleNamespace(num_transitions_per_env=4, num_envs=64, **{k: v.to(DEV).contiguous() for k, v in vars(st).items() if torch.is_tensor(v)})
    rng = np.random.default_rng(1)
    m = module_from_layers(make_layers(rng, [10, 16, 2]), make_layers(rng, [10, 8, 2]), torch.float32, weight=1.0).to(DEV)
    results = []
    for with_rnd in (False, True, True):
        rnd = HipRND(copy.deepcopy(m), num_learning_epochs=2, num_mini_batches=2, max_rows_per_minibatch=128) if with_rnd else None
        alg = HipPPO(copy.deepcopy(pol).to(DEV), num_learning_epochs=2, num_mini_batches=2, **({"rnd": rnd} if with_rnd else {}))
        out = alg.update(dev_st, torch.Generator(device=DEV).manual_seed(3))
        results.append((out, alg.flat("parameters").cpu(), alg.flat("exp_avg_sq").cpu(), rnd.flat("parameters").cpu() if with_rnd else None))
        alg.close()
        if rnd is not None:
            rnd.close()
    (o0, p0, v0, _), (o1, p1, v1, r1), (o2, p2, v2, r2) = results
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert set(o1) - set(o0) == {"rnd_loss"} and {k: v for k, v in o1.items() if k != "rnd_loss"} == o0 and o1["rnd_loss"] > 0
    assert o1 == o2 and torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(p1.view(torch.int32), p2.view(torch.int32))
    assert not torch.equal(r1, torch.cat([p.detach().reshape(-1) for p in m.predictor.parameters()]).cpu())


def _runner(monkeypatch, learner, rnd_cfg):
    from robot_lab_amd import shims
    from robot_lab_amd.env import ManagerBasedRLEnv

    shims.install()
    from rsl_rl.runners import OnPolicyRunner

    monkeypatch.setenv("RL_LEARNER", learner)
    cfg = dict(seed=3, num_steps_per_env=T, save_interval=100, policy=dict(class_name="ActorCritic", init_noise_std=1.0, activation="elu"),
               algorithm=dict(class_name="PPO", num_mini_batches=4, num_learning_epochs=2, rnd_cfg=rnd_cfg),
               obs_groups={"policy": ["policy"], "critic": ["critic"], "rnd_state": ["critic"]})
    env = types.SimpleNamespace(unwrapped=ManagerBasedRLEnv(A1F, num_envs=N, seed=3, device=DEV))
    return OnPolicyRunner(env, cfg, log_dir=None, device=DEV)


@pytest.mark.parametrize("src,dst", [("hip", "torch"), ("torch", "hip")])
def test_checkpoints_cross_the_learners(src, dst, monkeypatch, tmp_path):
    import torch

    cfg = {k: v for k, v in RND_FULL.items()}
    one = _runner(monkeypatch, src, cfg)
    assert one.trainer.rnd.group == "critic" and (one.trainer.rnd_learner is not None) == (src == "hip")
    one.learn(2)
    out = one.trainer.iterate()
    assert {"rnd_loss", "mean_intrinsic_reward", "mean_extrinsic_reward", "rnd_weight"} <= set(out) and out["rnd_loss"] > 0 and out["mean_intrinsic_reward"] > 0
    assert out["mean_reward"] == pytest.approx(out["mean_intrinsic_reward"] + out["mean_extrinsic_reward"], abs=1e-6)
    assert out["rnd_weight"] == pytest.approx(0.05)  # 12 calls: past the linear schedule's end
    path = str(tmp_path / "model.pt")
    one.save(path)
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert {k.split(".")[0] for k in d["rnd_state_dict"]} == {"predictor", "target", "state_normalizer", "reward_normalizer"}
    assert int(d["rnd_state_dict"]["state_normalizer.count"]) == 3 * T * N and int(d["rnd_state_dict"]["reward_normalizer.emp_norm.count"]) == 3 * T * N
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(tuple(v.shape))) for k, v in d["rnd_state_dict"].items() if k.startswith("predictor.")])
    ref_opt.load_state_dict(d["rnd_optimizer_state_dict"])  # torch.optim.Adam's layout
    assert int(float(d["rnd_optimizer_state_dict"]["state"][0]["step"])) == 3 * 2 * 4
    two = _runner(monkeypatch, dst, cfg)
    two.load(path)
    assert (two.trainer.rnd_learner is not None) == (dst == "hip")
    a, b = one.trainer.rnd_state_dict(), two.trainer.rnd_state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    oa, ob = one.trainer.rnd_optimizer_state_dict(), two.trainer.rnd_optimizer_state_dict()
    assert oa["param_groups"][0]["lr"] == ob["param_groups"][0]["lr"] and set(oa["state"]) == set(ob["state"])
    for i in oa["state"]:
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oa["state"][i][k].cpu(), ob["state"][i][k].cpu()), (i, k)
        assert float(oa["state"][i]["step"]) == float(ob["state"][i]["step"])
    x = one.env.unwrapped.get_observations()["critic"].clone()
    ya, yb = one.trainer.rnd_device.predictor(x).clone(), two.trainer.rnd_device.predictor(x).clone()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))
    out = two.trainer.iterate()  # the resumed training runs
    assert np.isfinite(out["rnd_loss"]) and np.isfinite(out["value_loss"])
    _close(one.trainer, two.trainer)
