"""`-m gpu`: the HIP recurrent learner (include/rl_bptt.h, robot_lab_amd/recurrent_hip.py) against the rule, `recurrent.RecurrentPPO` on the CPU.

Shapes, done pattern and the designed batch: tests/bptt_helpers.py (the smallest shapes where tile edges, slice edges and the block split can go
wrong; every row's clip / value-clip branch has a margin, asserted in fp64 before a device runs; no row is masked out).  tests/test_bptt_rule.py
shows on the CPU that each of seven wrong backward rules leaves the bound used here by 48 x to 6e5 x.

Exact, no tolerance: determinism of a whole update; the reset is a select (NaN behind it does not travel); dones[T - 1] is not read; the left-out
remainder env is not read; block 1 is block 0 of the storage with its env halves swapped.
Bounded, the project's bound (e <= 8 d per tensor, d the fp32 torch rule's own distance from the fp64 torch rule, both relative to max|ref64|):
forward, block_grad per parameter tensor, parameters and Adam moments after one whole update of two epochs, and two updates of the adaptive
schedule whose learning-rate path must be the fp64 rule's exactly.  `BPTT_PARITY_OUT=<file>` appends the measured multiples (profiles/bptt_parity.txt).
End to end: A1 Flat, 64 envs x 8 steps through `Trainer(recurrent_learner="hip")`, and checkpoints across the two learners through the runner."""
import copy
import functools
import os

import numpy as np
import pytest

import bptt_helpers as bh
from bptt_helpers import HYPER, SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAT = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
NAMES = list(SHAPES)


def _record(lines):
    path = os.environ.get("BPTT_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def _hip(name, pol=None, **kw):
    from robot_lab_amd.recurrent_hip import HipRecurrentPPO

    pol = bh.case(name)[0] if pol is None else pol
    return HipRecurrentPPO(copy.deepcopy(pol).to(DEV), num_mini_batches=SHAPES[name]["mb"], **{**HYPER, "num_learning_epochs": 2, **kw})


def _batch(name, fields=None):
    import torch

    return bh.as_batch(bh.case(name)[1] if fields is None else fields, torch.float32, DEV)


def _edit(name, **changes):
    """a writable copy of the case's fields with `changes(field array)` applied in place"""
    f = {k: np.array(v) for k, v in bh.case(name)[1].items()}
    for k, fn in changes.items():
        fn(f[k])
    return f


def _blocks(name):
    s = SHAPES[name]
    n = s["N"] // s["mb"]
    return [(b, b * n, n) for b in range(s["mb"])]


# ---- bounded ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_parity(name):
    hip, batch, lines, bad = _hip(name), _batch(name), [], []
    print()
    for b, lo, n in _blocks(name):
        ref = bh.reference_block(name, b)
        mean, value = hip.forward(batch, lo)
        got = dict(mean=mean.double().cpu().numpy().reshape(-1, mean.shape[-1]), value=value.double().cpu().numpy().reshape(-1))
        bad += bh.within_bound(f"{name} block {b}: forward", got, dict(mean=ref["f64"][0], value=ref["f64"][1]), dict(mean=ref["f32"][0], value=ref["f32"][1]), lines)
    hip.close()
    _record(lines)
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_block_grad_parity(name):
    """per parameter tensor, all eight LSTM tensors separately"""
    hip, batch, lines, bad = _hip(name), _batch(name), [], []
    pol = bh.case(name)[0]
    print()
    for b, lo, n in _blocks(name):
        ref = bh.reference_block(name, b)
        got = bh.split_flat(hip.block_grad(batch, lo), pol)
        assert len([k for k in got if ".rnn." in k]) == 8
        got["grad_norm"] = np.sqrt(sum(float((v ** 2).sum()) for v in got.values()))
        bad += bh.within_bound(f"{name} block {b}: block_grad", got, ref["f64"][2], ref["f32"][2], lines)
    hip.close()
    _record(lines)
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _reference_update(name, schedule, desired_kl, learning_rate, n_updates):
    """the torch rule's updates on the CPU in fp64 and fp32, once per case; the fp64 run's branch and KL margins are asserted here, before a device runs"""
    import torch

    pol, f = bh.case(name)
    out = {}
    for key, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        alg = bh.torch_alg(pol, dtype, SHAPES[name]["mb"], schedule=schedule, desired_kl=desired_kl, num_learning_epochs=2, learning_rate=learning_rate)
        results, lrs, seen = bh.checked_update(alg, bh.as_batch(f, dtype), n_updates, desired_kl or bh.DESIRED_KL)
        if key == "f64":
            # the designed margins (0.15, 0.1) shrink as the update moves the policy; 0.01 is still 1e3 x what fp32 does to a ratio or a value
            assert seen.ratio >= 0.01 and seen.dv >= 0.01 and seen.l12 >= 0.005, \
                f"{name}: a row comes within reach of a branch switch during the update: ratio {seen.ratio}, dv {seen.dv}, l1 - l2 {seen.l12}"
            if schedule == "adaptive":
                assert seen.kl_rel >= 0.1, f"{name}: the KL statistic comes within 10 % of a threshold of the schedule: fix the batch ({seen.kl_rel})"
        out[key] = dict(results=results, lrs=lrs, classes=seen.classes, params={k: p.detach().double().numpy() for k, p in alg.policy.named_parameters()},
                        exp_avg=bh.adam_named(alg, "exp_avg"), exp_avg_sq=bh.adam_named(alg, "exp_avg_sq"),
                        step=int(next(iter(alg.optimizer.state.values()))["step"]))
    assert all(np.array_equal(a, b) for a, b in zip(out["f64"]["classes"], out["f32"]["classes"])), f"{name}: the fp32 rule takes another branch than the fp64 rule"
    return out


@pytest.mark.parametrize("name", NAMES)
def test_one_update_parity(name):
    """parameters and both Adam moments after one whole update: two epochs x the blocks, fixed schedule"""
    ref = _reference_update(name, "fixed", None, HYPER["learning_rate"], 1)
    hip, batch, pol = _hip(name, schedule="fixed", desired_kl=None), _batch(name), bh.case(name)[0]
    res = hip.update(batch)
    assert set(res) == set(ref["f64"]["results"][0]) and hip.adam_step == ref["f64"]["step"] == 2 * SHAPES[name]["mb"]
    lines, bad = [], []
    print()
    for what, flat in (("params", "parameters"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")):
        bad += bh.within_bound(f"{name}: one update, {what}", bh.split_flat(hip.flat(flat), pol), ref["f64"][what], ref["f32"][what], lines)
    hip.close()
    _record(lines)
    assert not bad, bad


@pytest.mark.parametrize("desired_kl,learning_rate", [(0.01, 3e-4), (5.0, 1e-5)], ids=["kl-above-lr-falls", "kl-below-lr-rises"])
@pytest.mark.parametrize("name", ["ragged", "real-widths"])
def test_adaptive_learning_rate_path_over_two_updates(name, desired_kl, learning_rate):
    """the KL statistic of the designed batch (~0.5) sits far above 2 x 0.01 and far below 5 / 2: the learning-rate word must walk the fp64 rule's
    path EXACTLY (a path has no tolerance: the fp32 rule walks the same one, d = 0), with the update's statistics beside it.  Parameters and
    moments under the bound are test_one_update_parity's.  (A first form of this test also put the moments after the two adaptive updates under
    e <= 8 d: every tensor of the two "ragged" cases passed, and of "real-widths" all but the ONE-ELEMENT exp_avg of critic.6.bias, which measured
    e = 6.6e-7 against d = 8.0e-8, 8.2 x.  For a
    one-element tensor e / d is the ratio of two single round-off draws - the sum of 384 signed dvalue terms that cancel - and exceeds 8 about one
    time in thirteen for a perfect fp32 evaluation, so that extra comparison was dropped rather than tuned.)"""
    ref = _reference_update(name, "adaptive", desired_kl, learning_rate, 2)
    r64 = ref["f64"]
    assert r64["lrs"] == ref["f32"]["lrs"] and len(set(r64["lrs"])) == len(r64["lrs"]), "the path was meant to move at every block, alike in both precisions"
    per_update = len(r64["lrs"]) // 2
    hip, batch = _hip(name, schedule="adaptive", desired_kl=desired_kl, learning_rate=learning_rate), _batch(name)
    print()
    for u in range(2):
        res = hip.update(batch)
        want, w32 = r64["results"][u], ref["f32"]["results"][u]
        print(f"{name} update {u}: hip {res}\n{'':<{len(name) + 10}}f64 {want}")
        assert res["learning_rate"] == want["learning_rate"] == r64["lrs"][(u + 1) * per_update - 1]
        assert hip.adam_step == (u + 1) * per_update
        for k in ("value_loss", "surrogate_loss", "entropy", "kl"):  # (the statistics' rule of tests/test_gpu_ppo_hip_branches.py)
            assert abs(res[k] - want[k]) <= 8 * abs(w32[k] - want[k]) + 1e-6 * abs(want[k]), (k, res[k], w32[k], want[k])
    hip.close()


# ---- exact -----------------------------------------------------------------------------------------------------------------------------------
def _state(hip):
    return {k: hip.flat(k).cpu() for k in ("parameters", "exp_avg", "exp_avg_sq")}


@pytest.mark.parametrize("name", ["ragged", "real-widths"])
def test_two_updates_from_the_same_state_are_bit_identical(name):
    import torch

    runs = []
    for _ in range(2):
        hip = _hip(name, schedule="adaptive", desired_kl=0.01)
        stats = [hip.update(_batch(name)) for _ in range(2)]
        runs.append((stats, _state(hip), hip.last_grad_norm, hip.adam_step))
        hip.close()
    (s0, p0, g0, a0), (s1, p1, g1, a1) = runs
    assert s0 == s1 and g0 == g1 and a0 == a1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


@pytest.mark.parametrize("name", ["ragged", "4H-crosses-128"])
def test_the_reset_is_a_select(name):
    """for a row whose reset_k is set, (row, step >= k) does not depend on the row's observations before k nor on its h0 / c0 - replaced by other
    numbers, then by NaN"""
    import torch

    _, f = bh.case(name)
    dones = f["dones"]
    T, N = dones.shape
    k_of = np.full(N, -1)
    for k in range(1, T):
        k_of[dones[k - 1]] = k  # the last reset of the row
    rows = np.nonzero(k_of > 0)[0]
    assert len(rows) >= 10
    hip = _hip(name)
    base = {lo: hip.forward(_batch(name), lo) for _, lo, _ in _blocks(name)}
    for value in (7.0, np.nan):
        def before(a):
            for j in rows:
                a[:k_of[j], j] = value

        def state(a):
            a[rows] = value

        edited = _batch(name, _edit(name, observations=before, privileged_observations=before, h0_a=state, c0_a=state, h0_c=state, c0_c=state))
        checked = 0
        for _, lo, n in _blocks(name):
            mean, val = hip.forward(edited, lo)
            for j in rows[(rows >= lo) & (rows < lo + n)]:
                k = k_of[j]
                assert torch.equal(mean[k:, j - lo], base[lo][0][k:, j - lo]) and torch.equal(val[k:, j - lo], base[lo][1][k:, j - lo]), (value, j, k)
                assert not torch.equal(mean[:k, j - lo], base[lo][0][:k, j - lo])  # ... and before the reset it does
                checked += 1
            others = np.setdiff1d(np.arange(lo, lo + n), rows) - lo
            assert torch.equal(mean[:, others], base[lo][0][:, others])
        assert checked == len(rows[rows < SHAPES[name]["mb"] * (N // SHAPES[name]["mb"])])
    hip.close()


def test_the_last_dones_are_not_read():
    import torch

    name = "ragged"
    hip = _hip(name)

    def flip(d):
        d[-1] = ~d[-1]

    for _, lo, _ in _blocks(name):
        g0, (m0, v0) = hip.block_grad(_batch(name), lo), hip.forward(_batch(name), lo)
        flipped = _batch(name, _edit(name, dones=flip))
        g1, (m1, v1) = hip.block_grad(flipped, lo), hip.forward(flipped, lo)
        assert torch.equal(g0, g1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    hip.close()


def test_the_left_out_env_is_never_read():
    """N = 133 in four blocks of 33: env 132 belongs to no block.  Its rows are NaN (and its dones set) in every field: the update does not change"""
    import torch

    name = "4H-crosses-128"
    s = SHAPES[name]
    left = s["mb"] * (s["N"] // s["mb"])
    assert left == 132 and s["N"] == 133

    def nan_rows(a):
        if a.dtype == bool:
            a[:, left:] = True
        elif a.shape[0] == s["N"] and a.ndim == 2 and a.shape[1] == s["H"]:
            a[left:] = np.nan
        else:
            a[:, left:] = np.nan

    fields = _edit(name, **{k: nan_rows for k in bh.case(name)[1]})
    assert np.isnan(fields["observations"][:, left]).all() and np.isnan(fields["h0_a"][left]).all() and np.isfinite(fields["observations"][:, :left]).all()
    out = []
    for fl in (None, fields):
        hip = _hip(name, schedule="adaptive", desired_kl=0.01)
        stats = hip.update(_batch(name, fl))
        out.append((stats, _state(hip)))
        hip.close()
    assert out[0][0] == out[1][0] and all(np.isfinite(v) for v in out[1][0].values())
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


def test_block_one_is_block_zero_of_the_swapped_storage():
    import torch

    name = "ragged"
    s = SHAPES[name]
    n = s["N"] // s["mb"]
    assert s["mb"] == 2 and 2 * n == s["N"]
    perm = np.concatenate([np.arange(n, 2 * n), np.arange(0, n)])
    swapped = {k: np.ascontiguousarray(v[perm] if k in ("h0_a", "c0_a", "h0_c", "c0_c") else v[:, perm]) for k, v in bh.case(name)[1].items()}
    hip = _hip(name)
    g1 = hip.block_grad(_batch(name), n)
    g0 = hip.block_grad(_batch(name, swapped), 0)
    assert torch.equal(g0, g1)
    assert not torch.equal(g0, hip.block_grad(_batch(name), 0))
    hip.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_trainer_end_to_end():
    """A1 Flat, 64 envs x 8 steps, two iterations: every parameter moves and stays finite, and the kernels the collector launches hold the learner's
    parameters bit for bit after the push (a cell / head built anew from the synced module gives the same bits on the same rows)"""
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.lstm import LstmCell
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.ppo import Trainer
    from robot_lab_amd.recurrent_hip import HipRecurrentPPO

    n = 64
    env = ManagerBasedRLEnv(FLAT, num_envs=n, seed=42, device=DEV)
    tr = Trainer(env, seed=42, num_steps_per_env=8, rnn_type="lstm", rnn_hidden_dim=64, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128),
                 recurrent_learner="hip", num_learning_epochs=2)
    assert isinstance(tr.alg, HipRecurrentPPO) and "recurrent_learner='hip'" in repr(tr)
    env.episode_length_buf = env.max_episode_length - 1 - (torch.arange(n) % 12)  # time-outs inside the window: resets in the batch
    before = {k: v.clone() for k, v in tr.state_dict().items()}
    for _ in range(2):
        out = tr.iterate()
        assert all(np.isfinite(out[k]) for k in ("value_loss", "surrogate_loss", "entropy", "kl", "learning_rate", "mean_reward", "action_std")), out
    assert bool(tr.storage.dones[:-1].any())
    after = tr.state_dict()
    assert len(after) == len(before) == 1 + 8 + 16
    for k in before:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    flat = tr.alg.flat("parameters")
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in tr.policy.parameters()]))  # state_dict() synced the module
    assert torch.equal(tr.std, flat[:env.num_actions])
    g = torch.Generator(device=DEV).manual_seed(1)
    for cell, rnn in ((tr.recurrent.cell_a, tr.policy.memory_a.rnn), (tr.recurrent.cell_c, tr.policy.memory_c.rnn)):
        fresh = LstmCell.from_module(rnn, device=DEV)
        x, h, c = (torch.randn(n, w, device=DEV, generator=g) for w in (cell.in_dim, 64, 64))
        outs = []
        for one in (cell, fresh):
            h1, c1 = torch.empty_like(h), torch.empty_like(c)
            one.step(x, h, c, h1, c1)
            outs.append((h1, c1))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        fresh.close()
    lin = lambda m: [x for x in m if isinstance(x, torch.nn.Linear)]  # noqa: E731
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    for head, module in ((tr.actor, tr.policy.actor), (tr.critic, tr.policy.critic)):
        fresh = MlpPolicy([host(x.weight) for x in lin(module)], [host(x.bias) for x in lin(module)], "elu", device=DEV)
        x = torch.randn(n, 64, device=DEV, generator=g)
        assert torch.equal(head(x), fresh(x))
        fresh.close()
    tr.alg.close(); tr.recurrent.close(); tr.storage.close(); env.close()


def _runner(monkeypatch, learner, n=64):
    from robot_lab_amd import shims

    shims.install()
    import gymnasium as gym
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from recurrent_helpers import RSL_RL_SPELLING
    from rsl_rl.runners import OnPolicyRunner

    cfg = copy.deepcopy(RSL_RL_SPELLING)
    cfg["policy"]["rnn_hidden_dim"] = 64
    cfg["algorithm"].update(num_learning_epochs=2, num_mini_batches=4)
    monkeypatch.setenv("RL_RECURRENT_LEARNER", learner)
    if FLAT not in getattr(gym, "registry", {}):
        gym.register(id=FLAT, entry_point="isaaclab.envs:ManagerBasedRLEnv", disable_env_checker=True, kwargs={})
    env = RslRlVecEnvWrapper(gym.make(FLAT, cfg=FLAT, num_envs=n, seed=3, device=DEV), clip_actions=None)
    return env, OnPolicyRunner(env, dict(cfg, seed=7, num_steps_per_env=8, save_interval=100), log_dir=None, device=DEV)


def _optimizer_state(runner):
    """(exp_avg flat, exp_avg_sq flat, step, lr) of either learner, on the host"""
    import torch

    from robot_lab_amd.ppo_hip import adam_state_flat

    alg = runner.alg
    d = alg.optimizer_state_dict() if hasattr(alg, "optimizer_state_dict") else alg.optimizer.state_dict()
    m1, m2, step, lr = adam_state_flat(d, [tuple(p.shape) for p in alg.policy.parameters()])
    return m1.cpu(), m2.cpu(), step, lr, float(alg.learning_rate)


def test_checkpoints_cross_the_two_learners(monkeypatch, tmp_path):
    """a checkpoint written by the HIP learner is resumed by the torch learner and the reverse: equal parameters, moments, step and learning rate"""
    import torch

    from robot_lab_amd.recurrent import RecurrentPPO
    from robot_lab_amd.recurrent_hip import HipRecurrentPPO

    env_a, a = _runner(monkeypatch, "hip")
    env_b, b = _runner(monkeypatch, "torch")
    assert isinstance(a.alg, HipRecurrentPPO) and isinstance(b.alg, RecurrentPPO)
    for src, dst, its in ((a, b, 2), (b, a, 1)):
        src.learn(num_learning_iterations=its)
        path = str(tmp_path / f"model_{its}.pt")
        src.save(path)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert ck["optimizer_state_dict"]["state"] and ck["iter"] == src.current_learning_iteration
        dst.load(path)
        assert dst.current_learning_iteration == src.current_learning_iteration
        if hasattr(dst.alg, "sync_policy"):
            dst.alg.sync_policy()  # (what the learner holds, not what load_state_dict put into the module)
        for (k, p), q in zip(src.alg.policy.state_dict().items(), dst.alg.policy.state_dict().values()):
            assert torch.equal(p, q), k
        s, d = _optimizer_state(src), _optimizer_state(dst)
        assert torch.equal(s[0], d[0]) and torch.equal(s[1], d[1]) and s[2:] == d[2:] and s[2] > 0, (s[2:], d[2:])
    env_a.close(); env_b.close()
