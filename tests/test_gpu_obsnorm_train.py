"""`-m gpu`: observation normalisation end to end - the collector's order of operations, the raw storage, both learners on the normalised batch,
checkpoints across the learners and the runner stand-in (robot_lab_amd/collect.py, ppo.py, obsnorm.py, shims/rsl_rl/runners).  The comparator is
the rule of robot_lab_amd.ppo (`EmpiricalNormalization`, `PPO.update`) in fp64; bounds are those of tests/test_gpu_obsnorm.py (state),
tests/test_gpu_policy_exact.py (the inference MLP) and tests/test_gpu_ppo_hip.py (the learner).  A1 Flat, 64 envs, 4 steps; one G1 case."""
import copy
import types

import numpy as np
import pytest

import obsnorm_helpers as oh
import policy_helpers as ph
from oracle.policy import mlp_forward
from ppo_helpers import DEV, cast as _cast, gen as _gen, perm as perm_of, split as _split, torch_learner as _torch_learner

pytestmark = pytest.mark.gpu
A1, G1 = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0", "RobotLab-Isaac-Velocity-Flat-Unitree-G1-v0"
T, N = 4, 64
BUFFERS = ("observations", "privileged_observations", "actions", "mu", "sigma", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages")


def _trainer(task=A1, n=N, seed=3, **kw):
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(task, num_envs=n, seed=seed, device=DEV)
    return Trainer(env, num_steps_per_env=T, seed=seed, **kw)


def _close(*trainers):
    for tr in trainers:
        tr.env.close()


def _np(t):
    return t.detach().cpu().numpy()


def _handle_state(h):
    mean, var, std, count = h.get_state()
    return dict(mean=_np(mean).reshape(-1), var=_np(var).reshape(-1), std=_np(std).reshape(-1), count=count)


def _storage_bits(st):
    import torch

    return {k: getattr(st, k).clone().view(torch.uint8 if k == "dones" else torch.int32) for k in BUFFERS}


def _assert_same_storage(a, b, what, only=BUFFERS):
    import torch

    for k in only:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} entries"


def _layers(seq):
    import torch

    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    return [_np(m.weight) for m in lin], [_np(m.bias) for m in lin]


@pytest.mark.parametrize("task,n", [(A1, N), (G1, 32)])
def test_one_collection_statistics_order_and_stored_mu(task, n):
    """After one collect(): count = T N in both groups; the state is the fp64 rule replayed over storage rows 1 .. T - 1 and the collector's
    current observations (the NEW observations of every step; the row after reset() never enters), within the kernels' bound; the stored mu
    of step t is the fp64 actor on the fp64-normalised raw row with the statistics of step t, within the inference MLP's bound."""
    tr = _trainer(task, n, actor_obs_normalization=True, critic_obs_normalization=True)
    assert "obs_normalization=['policy', 'critic']" in repr(tr)
    tr.collector.collect()
    st = tr.storage
    ws, bs = _layers(tr.policy.actor)
    for h, key, rows in zip(tr.normalizers, ("policy", "critic"), (st.observations, st.privileged_observations)):
        rows = _np(rows)
        seen = [rows[t] for t in range(1, T)] + [_np(tr.collector.obs[key])]
        got = _handle_state(h)
        assert got["count"] == T * n
        ref, emu, per_step = oh.fresh(rows.shape[-1]), oh.fresh(rows.shape[-1], oh.F), []
        for x in seen:
            per_step.append((ref, emu))
            ref, emu = oh.rule(ref, x, np.float64), oh.rule(emu, x, oh.F)
        for k in oh.VECTORS:
            e, e32 = oh.vector_error(got, ref, k), oh.vector_error(emu, ref, k)
            print(f"[obsnorm-train] {task} {key} {k}: E = {e:.3e}, E32 = {e32:.3e}, ratio {e / e32:.3f}")
            assert e <= oh.K_STATE * e32, (key, k, e, e32)
        if key == "policy":
            for t, (r64, r32) in enumerate(per_step):
                want = mlp_forward((rows[t].astype(np.float64) - r64["mean"]) / (r64["std"] + oh.EPS), ws, bs, "elu")
                x32 = oh.apply_f32(rows[t], r32["mean"], r32["std"])
                ph.assert_fp32_bound(_np(st.mu[t]), x32, ws, bs, "elu", f"{task} stored mu of step {t}", want)
    _close(tr)


def _blind(tr):
    """the actor's last layer without weights: mean = bias whatever the network sees, so the trajectory does not depend on the normalisation"""
    import torch

    with torch.no_grad():
        tr.policy.actor[-1].weight.zero_()
    if tr.learner == "hip":
        tr.alg.load_from(tr.policy)
    tr.push_parameters()


def test_the_storage_keeps_the_raw_rows():
    """two trainers on the same seed, normalisation on and off, both with an actor whose output ignores its input: the same actions, so the
    same trajectory - every stored observation, privileged observation, action, reward and done flag is bit-identical (the normaliser
    changed no entry of the slot), while the values (the critic DOES see normalised rows) differ"""
    import torch

    on, off = _trainer(actor_obs_normalization=True, critic_obs_normalization=True), _trainer()
    for tr in (on, off):
        _blind(tr)
        tr.collector.collect()
    a, b = _storage_bits(on.storage), _storage_bits(off.storage)
    _assert_same_storage(a, b, "normalisation on / off", ("observations", "privileged_observations", "actions", "mu", "rewards", "dones"))
    assert not torch.equal(a["values"], b["values"])
    assert torch.equal(on.collector.obs["policy"], off.collector.obs["policy"])
    _close(on, off)


@pytest.mark.parametrize("flags", [dict(actor_obs_normalization=True, critic_obs_normalization=True), dict(critic_obs_normalization=True)])
def test_eager_and_graph_collection_are_bit_identical(flags):
    import torch

    eager, graph = _trainer(use_graph=False, **flags), _trainer(use_graph=True, **flags)
    for it in range(3):  # the graph trainer: eager once, captured and replayed, replayed
        for tr in (eager, graph):
            tr.collector.collect()
        _assert_same_storage(_storage_bits(eager.storage), _storage_bits(graph.storage), f"iteration {it}")
        for he, hg in zip(eager.normalizers, graph.normalizers):
            if he is not None:
                se, sg = _handle_state(he), _handle_state(hg)
                assert se["count"] == sg["count"] == (it + 1) * T * N
                for k in oh.VECTORS:
                    oh.assert_bits_equal(sg[k], se[k], f"iteration {it}, {k}")
    assert graph.collector._graph is not None and eager.collector._graph is None
    _close(eager, graph)


def test_flags_off_is_the_trainer_that_never_heard_of_them():
    plain, off = _trainer(), _trainer(actor_obs_normalization=False, critic_obs_normalization=False)
    assert off.normalizers is None and off.collector.normalizers is None and "obs_normalization" not in repr(off)
    assert sorted(off.state_dict()) == sorted(plain.state_dict())
    for it in range(2):
        for tr in (plain, off):
            tr.collector.collect()
        _assert_same_storage(_storage_bits(plain.storage), _storage_bits(off.storage), f"iteration {it}")
    _close(plain, off)


@pytest.mark.parametrize("flags", [dict(actor_obs_normalization=True), dict(critic_obs_normalization=True),
                                   dict(actor_obs_normalization=True, critic_obs_normalization=True)], ids=["actor", "critic", "both"])
def test_both_learners_on_the_same_collected_batch(flags):
    """The HIP learner reads the batch normalised by rl_obsnorm_apply; the comparator is `ppo.PPO` in fp64 on the RAW stored rows with the
    normaliser MODULES in the policy (fp32 beside it for the yardstick).  Gradient of the first mini-batch: e <= 8 d per tensor; parameters
    after one update (fixed schedule: 20 steps on 64-row mini-batches): q999 <= max(8 q999 of torch-fp32, one spacing), max <= the
    displacement Adam allows - the bounds of tests/test_gpu_ppo_hip.py.  The torch learner inside the Trainer reads the same pre-normalised
    batch: its update equals `PPO.update` on the raw rows bit for bit on the statistics (the exact apply test pins the rows)."""
    import torch

    tr = _trainer(learner="hip", schedule="fixed", **flags)
    tr.collector.collect()
    tr._batch.normalize()
    tr.sync_normalizers()
    torch.cuda.synchronize()
    pol = copy.deepcopy(tr.policy).cpu()
    for m, h in zip((pol.actor_obs_normalizer, pol.critic_obs_normalizer), tr.normalizers):
        assert (h is None) == isinstance(m, torch.nn.Identity)
        if h is not None:
            assert int(m.count) == T * N and float(m._mean.abs().max()) > 0
    raw = types.SimpleNamespace(num_transitions_per_env=T, num_envs=N, **{k: getattr(tr.storage, k).clone() for k in BUFFERS if k != "dones"})
    B, MB = T * N, T * N // 4
    idx = perm_of(B)[:MB]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = _torch_learner(pol, dtype, num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30, schedule="fixed")
        alg.update(_cast(raw, dtype, rows=idx), _gen(5))
        ref[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}
    g_hip = _split(tr.alg.minibatch_grad(tr._batch, idx), pol)
    bad = []
    print(f"\n{sorted(flags)}\n{'tensor':<18}{'max|g64|':>12}{'e (hip)':>12}{'d (torch32)':>13}{'e/d':>8}")
    for n, g64 in ref[torch.float64].items():
        scale = g64.abs().max().item()
        e = (g_hip[n].reshape(g64.shape) - g64).abs().max().item() / scale
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        print(f"{n:<18}{scale:12.4e}{e:12.3e}{d:13.3e}{e / d if d else float('inf'):8.2f}")
        if not e <= 8 * d:
            bad.append((n, e, d))
    assert not bad, f"gradient error above 8 x the fp32 torch learner's: {bad}"
    # one update
    a64, a32 = _torch_learner(pol, torch.float64, schedule="fixed"), _torch_learner(pol, torch.float32, schedule="fixed")
    a64.update(_cast(raw, torch.float64), _gen())
    a32.update(_cast(raw, torch.float32), _gen())
    tr.alg.update(tr._batch, _gen())
    out = tr.alg.store_into(copy.deepcopy(tr.policy))
    torch.cuda.synchronize()
    displacement = float(sum(a64.lr_path))
    assert len(a64.lr_path) == 20
    bad = []
    for (n, p64), (_, p32), (_, ph_) in zip(a64.policy.named_parameters(), a32.policy.named_parameters(), out.named_parameters()):
        p64, p32, ph_ = (p.detach().double().cpu() for p in (p64, p32, ph_))
        dh, d32 = (ph_ - p64).abs().flatten(), (p32 - p64).abs().flatten()
        qh, q32 = torch.quantile(dh, 0.999).item(), torch.quantile(d32, 0.999).item()
        ulp = float(np.spacing(np.float32(p64.abs().max().item())))
        print(f"{n:<18}{qh:12.3e}{q32:14.3e}{dh.max().item():12.3e}{d32.max().item():13.3e}")
        if not qh <= max(8 * q32, ulp):
            bad.append((n, "q999", qh, q32))
        if not dh.max().item() <= displacement:
            bad.append((n, "max", dh.max().item(), displacement))
    assert not bad, bad
    _close(tr)


def test_the_torch_learner_in_the_trainer_reads_the_same_rows_as_the_rule():
    """`Trainer(learner="torch")` hands `PPO.update` the pre-normalised batch; the rule is `PPO.update` on the raw rows through the modules.
    Same rows bit for bit (torch's fp32 (x - mean) / (std + eps) on the device against rl_obsnorm_apply), so the same update: checked on the
    rows and on the parameters after one iterate() against a twin that runs the rule."""
    import torch

    a, b = _trainer(actor_obs_normalization=True, critic_obs_normalization=True), _trainer(actor_obs_normalization=True, critic_obs_normalization=True)
    for tr in (a, b):
        tr.collector.collect()
        tr._batch.normalize()
        tr.sync_normalizers()
    for key, mod in (("observations", a.policy.actor_obs_normalizer), ("privileged_observations", a.policy.critic_obs_normalizer)):
        want = mod(getattr(a.storage, key))
        assert torch.equal(getattr(a._batch, key).view(torch.int32), want.view(torch.int32)), key
    a.alg.update(a._batch, a.gen)    # the Trainer's path
    b.alg.update(b.storage, b.gen)   # the rule: raw rows through the modules
    for (n, p), (_, q) in zip(a.policy.named_parameters(), b.policy.named_parameters()):
        torch.testing.assert_close(p, q, rtol=0, atol=0, msg=n)
    _close(a, b)


def _runner(monkeypatch, learner, n=N, **policy_flags):
    from robot_lab_amd import shims
    from robot_lab_amd.env import ManagerBasedRLEnv

    shims.install()
    from rsl_rl.runners import OnPolicyRunner

    monkeypatch.setenv("RL_LEARNER", learner)
    cfg = dict(seed=3, num_steps_per_env=T, save_interval=100, policy=dict(class_name="ActorCritic", init_noise_std=1.0, activation="elu", **policy_flags),
               algorithm=dict(class_name="PPO", num_mini_batches=4))
    env = types.SimpleNamespace(unwrapped=ManagerBasedRLEnv(A1, num_envs=n, seed=3, device=DEV))
    return OnPolicyRunner(env, cfg, log_dir=None, device=DEV)


BOTH = dict(actor_obs_normalization=True, critic_obs_normalization=True)


@pytest.mark.parametrize("src,dst", [("hip", "torch"), ("torch", "hip")])
def test_checkpoints_cross_the_learners(src, dst, monkeypatch, tmp_path):
    import torch

    one = _runner(monkeypatch, src, **BOTH)
    one.learn(2)
    path = str(tmp_path / "model.pt")
    one.save(path)
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert {f"{g}_obs_normalizer.{k}" for g in ("actor", "critic") for k in ("_mean", "_var", "_std", "count")} <= set(d["model_state_dict"])
    assert int(d["model_state_dict"]["actor_obs_normalizer.count"]) == 2 * T * N
    two = _runner(monkeypatch, dst, **BOTH)
    two.load(path)
    assert type(two.alg).__name__ == ("HipPPO" if dst == "hip" else "PPO")
    for h1, h2, name in zip(one.trainer.normalizers, two.trainer.normalizers, ("actor_obs_normalizer", "critic_obs_normalizer")):
        s1, s2 = _handle_state(h1), _handle_state(h2)
        assert s1["count"] == s2["count"] == 2 * T * N
        for k in oh.VECTORS:
            oh.assert_bits_equal(s2[k], s1[k], f"{src} -> {dst}, {name} {k}")
            oh.assert_bits_equal(_np(getattr(getattr(two.alg.policy, name), "_" + k)).reshape(-1), s1[k], f"{src} -> {dst}, module {name} {k}")
    obs = one.env.unwrapped.get_observations()["policy"].clone()
    y1, y2 = one.get_inference_policy()(obs).clone(), two.get_inference_policy()({"policy": obs}).clone()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))
    out = two.trainer.iterate()  # the resumed training runs
    assert np.isfinite(out["value_loss"]) and _handle_state(two.trainer.normalizers[0])["count"] == 3 * T * N
    _close(one.trainer, two.trainer)


@pytest.mark.parametrize("flags", [dict(actor_obs_normalization=True), dict(critic_obs_normalization=True), BOTH], ids=["actor", "critic", "both"])
def test_the_runner_takes_the_flags(flags, monkeypatch, tmp_path):
    """`runner.alg.policy.actor_obs_normalizer` is there and current after learn(); the inference policy applies the actor's statistics
    without moving them; the shim's exported TorchScript module (normaliser + actor) and the inference policy both sit within the inference
    MLP's bound of the fp64 oracle on the fp64-normalised rows."""
    import torch

    from robot_lab_amd.ppo import EmpiricalNormalization

    runner = _runner(monkeypatch, "torch", **flags)
    from isaaclab_rl.rsl_rl import export_policy_as_jit  # (the shims are installed by _runner)

    runner.learn(2)
    pol = runner.alg.policy
    for name, on, h in (("actor_obs_normalizer", "actor_obs_normalization" in flags, runner.trainer.normalizers[0]),
                        ("critic_obs_normalizer", "critic_obs_normalization" in flags, runner.trainer.normalizers[1])):
        mod = getattr(pol, name)
        assert isinstance(mod, EmpiricalNormalization if on else torch.nn.Identity) and (h is not None) == on
        if on:
            s = _handle_state(h)
            assert int(mod.count) == s["count"] == 2 * T * N
            for k in oh.VECTORS:
                oh.assert_bits_equal(_np(getattr(mod, "_" + k)).reshape(-1), s[k], f"{name} {k} after learn()")
    before = [None if h is None else _handle_state(h) for h in runner.trainer.normalizers]
    obs = runner.env.unwrapped.get_observations()["policy"].clone()
    policy = runner.get_inference_policy(device=DEV)
    got = _np(policy(obs).clone())
    for h, b in zip(runner.trainer.normalizers, before):
        if h is not None:
            s = _handle_state(h)
            assert s["count"] == b["count"]
            for k in oh.VECTORS:
                oh.assert_bits_equal(s[k], b[k], f"inference moved {k}")
    normalizer = pol.actor_obs_normalizer if "actor_obs_normalization" in flags else None  # play.py:223-233
    export_policy_as_jit(pol, normalizer=normalizer, path=str(tmp_path), filename="policy.pt")
    jit = _np(torch.jit.load(str(tmp_path / "policy.pt"))(obs.cpu()))
    ws, bs = _layers(pol.actor)
    x = _np(obs)
    if normalizer is not None:
        m, s = _np(normalizer._mean).reshape(-1), _np(normalizer._std).reshape(-1)
        want = mlp_forward((x.astype(np.float64) - m) / (s.astype(np.float64) + oh.EPS), ws, bs, "elu")
        x = oh.apply_f32(x, m, s)
    else:
        want = mlp_forward(x, ws, bs, "elu")
    ph.assert_fp32_bound(got, x, ws, bs, "elu", f"inference policy {sorted(flags)}", want)
    ph.assert_fp32_bound(jit, x, ws, bs, "elu", f"exported module {sorted(flags)}", want)
    _close(runner.trainer)


def test_refusals(monkeypatch, tmp_path):
    import torch

    from robot_lab_amd.collect import Collector
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1, num_envs=N, seed=3, device=DEV)
    with pytest.raises(NotImplementedError, match="symmetry"):
        Trainer(env, num_steps_per_env=T, symmetry="lr", actor_obs_normalization=True)
    with pytest.raises(NotImplementedError, match="2 ranks"):
        Trainer(env, num_steps_per_env=T, critic_obs_normalization=True, group=types.SimpleNamespace(world_size=2, enabled=True))
    tr = Trainer(env, num_steps_per_env=T, seed=3, **BOTH)
    with pytest.raises(NotImplementedError, match="overlap"):
        Collector(env, tr.actor, tr.critic, tr.storage, tr.std, overlap=True, normalizers=tr.normalizers)
    env.close()
    # a checkpoint with normaliser keys into a runner without the flags, and the reverse: load_state_dict's own error
    on, off = _runner(monkeypatch, "torch", **BOTH), _runner(monkeypatch, "hip")
    p_on, p_off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    on.save(p_on)
    off.save(p_off)
    with pytest.raises(RuntimeError, match="Unexpected key.*obs_normalizer"):
        off.load(p_on)
    with pytest.raises(RuntimeError, match="Missing key.*obs_normalizer"):
        on.load(p_off)
    # rsl_rl's deprecated runner-level spelling stays refused (tests/test_distributed_train.py pins it), with the two flags named
    from rsl_rl.runners import OnPolicyRunner

    with pytest.raises(NotImplementedError, match="actor_obs_normalization=True and policy.critic_obs_normalization=True"):
        OnPolicyRunner(types.SimpleNamespace(unwrapped=None), dict(on.cfg, empirical_normalization=True), device=DEV)
    _close(on.trainer, off.trainer)


def test_a1_learns_to_track_velocity_commands_with_normalisation():
    """tests/test_gpu_train.py::test_a1_learns_to_track_velocity_commands with both groups normalised (HIP learner): same envs, iterations
    and criterion"""
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    n, iters = 2048, 60
    env = ManagerBasedRLEnv(A1, num_envs=n, seed=42, device=DEV)
    tr = Trainer(env, seed=42, learner="hip", **BOTH)
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (n,), generator=torch.Generator().manual_seed(0))
    rew, done = [], []
    for _ in range(iters):
        out = tr.iterate()
        rew.append(out["mean_reward"])
        done.append(out["done_rate"])
        assert np.isfinite(out["value_loss"]) and np.isfinite(out["surrogate_loss"])
    first, last = float(np.mean(rew[:5])), float(np.mean(rew[-5:]))
    print(f"\n[train, normalised] A1 Flat {n} envs: reward/step {first:+.4f} -> {last:+.4f}; done/step {np.mean(done[:5]):.4f} -> {np.mean(done[-5:]):.4f}; "
          f"std {out['action_std']:.3f}; lr {out['learning_rate']:.1e}")
    assert last > first + 0.5 * abs(first) or last > first + 0.01, "the mean step reward did not improve in 60 PPO iterations"
    assert np.mean(done[-5:]) <= np.mean(done[:5]) + 1e-3, "episodes end more often than at the start: the policy is falling over more"
    sd = tr.state_dict()
    assert int(sd["actor_obs_normalizer.count"]) == int(sd["critic_obs_normalizer.count"]) == iters * 24 * n
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    env.close()
