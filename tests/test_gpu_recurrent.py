"""Recurrent policies on the MI355X, end to end: the recurrent `Collector` on the real env (resets, state record, bootstrap, the fp64
replay of the rule, captured replay against the eager loop), the `Trainer` and the `OnPolicyRunner` stand-in (learning, checkpoints,
both cfg spellings, the stateful inference policy) and every device-side refusal.  The cell kernel alone: tests/test_gpu_lstm_exact.py;
the rule on the CPU: tests/test_recurrent.py."""
import copy

import numpy as np
import pytest

import recurrent_helpers as rh

REFERENCE_SPELLING, RSL_RL_SPELLING = rh.REFERENCE_SPELLING, rh.RSL_RL_SPELLING

pytestmark = pytest.mark.gpu
DEV = rh.DEV
FLAT = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
N, T, H = 64, 24, 256


def _module(od, cd, A):
    import torch

    from robot_lab_amd.recurrent import ActorCriticRecurrent

    torch.manual_seed(5)
    return ActorCriticRecurrent(od, cd, A, rnn_hidden_dim=H, init_noise_std=0.3)


def _setup(use_graph, **collector_kw):
    """A1 Flat, 64 envs, T = 24; every fourth env is 0 .. 15 steps from its time-out, envs 1 .. 3 are 22 .. 24 steps from it (one of them ends on
    the window's last step)"""
    import torch
    from torch import nn

    from robot_lab_amd.collect import Collector
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.lstm import LstmCell, RecurrentState
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.rollout import RolloutStorage

    env = ManagerBasedRLEnv(FLAT, num_envs=N, seed=11, device=DEV)
    obs, _ = env.reset()
    ep = torch.zeros(N, dtype=torch.long)
    idx = torch.arange(0, N, 4)
    ep[idx] = env.max_episode_length - 1 - (idx // 4)
    ep[1:4] = env.max_episode_length - torch.tensor([22, 23, 24])
    env.episode_length_buf = ep
    od, cd, A = obs["policy"].shape[1], obs["critic"].shape[1], env.num_actions
    pol = _module(od, cd, A)
    lin = lambda m: [x for x in m if isinstance(x, nn.Linear)]  # noqa: E731
    host = lambda t: t.detach().numpy()  # noqa: E731
    actor = MlpPolicy([host(x.weight) for x in lin(pol.actor)], [host(x.bias) for x in lin(pol.actor)], "elu", device=DEV)
    critic = MlpPolicy([host(x.weight) for x in lin(pol.critic)], [host(x.bias) for x in lin(pol.critic)], "elu", device=DEV)
    rec = RecurrentState(LstmCell.from_module(pol.memory_a.rnn, device=DEV), LstmCell.from_module(pol.memory_c.rnn, device=DEV), N, T)
    st = RolloutStorage(N, T, od, cd, A, seed=3, device=DEV)
    std = torch.full((A,), 0.3, device=DEV)
    return env, pol, st, rec, Collector(env, actor, critic, st, std, use_graph=use_graph, recurrent=rec, **collector_kw)


def _snapshot(st, rec):
    import torch

    torch.cuda.synchronize()
    out = {k: getattr(st, k).clone() for k in ("observations", "privileged_observations", "actions", "mu", "values", "rewards", "dones", "returns", "advantages")}
    out.update({k: getattr(rec, k).clone() for k in ("h_a", "c_a", "h_c", "c_c", "reset")})
    (ha, ca), (hc, cc) = rec.state()
    out.update(state_ha=ha.clone(), state_ca=ca.clone(), state_hc=hc.clone(), state_cc=cc.clone())
    return out


@pytest.fixture(scope="module")
def two_iterations():
    """two eager iterations of the recurrent collector, snapshots after each (shared, read only)"""
    env, pol, st, rec, col = _setup(False)
    snaps = []
    for _ in range(2):
        col.collect()
        snaps.append(_snapshot(st, rec))
    last_obs = {k: v.clone() for k, v in col.obs.items()}
    yield pol, snaps, last_obs, (env, st, rec, col)
    rec.close(); st.close(); env.close()


def test_dones_fall_inside_the_window(two_iterations):
    _, snaps, _, _ = two_iterations
    d = snaps[0]["dones"]
    frac = float(d.any(0).float().mean())
    print(f"[recurrent collect] {100 * frac:.1f} % of the envs see a done in the first iteration; {int(d[T - 1].sum())} on its last step")
    assert 0.05 <= frac <= 0.50, frac
    assert bool(d[T - 1].any()), "no env ends on the window's last step: the carry into the next iteration would go untested"
    assert bool(d[:T - 1].any())


def test_saved_state_is_zero_exactly_behind_a_done(two_iterations):
    import torch

    _, snaps, _, _ = two_iterations
    for s in snaps:
        d = s["dones"]
        for k in ("h_a", "c_a", "h_c", "c_c"):
            nxt = s[k][1:]  # the state steps 1 .. T - 1 started from
            on = d[:-1].unsqueeze(-1).expand_as(nxt)
            assert bool((nxt[on].view(torch.int32) == 0).all()), f"{k}: a row behind a done does not start from zero"
            rows_nonzero = (nxt != 0).any(-1)
            assert bool(rows_nonzero[~d[:-1]].all()), f"{k}: a row that was not reset starts from a zero state"


def test_last_dones_reset_the_first_step_of_the_next_iteration(two_iterations):
    import torch

    _, (first, second), _, _ = two_iterations
    carry = first["dones"][T - 1]
    assert torch.equal(first["reset"].bool(), carry)
    for k, state in (("h_a", "state_ha"), ("c_a", "state_ca"), ("h_c", "state_hc"), ("c_c", "state_cc")):
        slot0 = second[k][0]
        assert bool((slot0[carry].view(torch.int32) == 0).all()), f"{k}: the last step's dones did not reset step 0 of the next iteration"
        assert torch.equal(slot0[~carry].view(torch.int32), first[state][~carry].view(torch.int32)), f"{k}: the state did not cross the iterations bit for bit"


def test_bootstrap_commits_nothing(two_iterations):
    import torch

    _, _, last_obs, (env, st, rec, col) = two_iterations
    before = [t.clone() for pair in rec.state() for t in pair]
    k = rec._k
    out = rec.bootstrap(last_obs["critic"], rec.reset).clone()
    torch.cuda.synchronize()
    after = [t for pair in rec.state() for t in pair]
    assert rec._k == k and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))
    assert bool(torch.isfinite(out).all()) and bool((out != 0).any())


def test_fp64_replay_of_the_rule_reproduces_the_stored_means_and_values(two_iterations):
    """`ActorCriticRecurrent` in fp64 over the stored observations, from the saved state of step 0, zeroed behind every done: the stored mu and values
    within M_BOUND x the distance of the same replay in fp32 (torch, CPU) from it.  The second iteration's replay also shows that obs_T entered
    the critic's memory once: its step 0 starts from a state that never saw it."""
    import torch

    pol, snaps, _, _ = two_iterations
    bad = []
    for it, s in enumerate(snaps):
        c = {k: v.cpu() for k, v in s.items()}
        d = c["dones"]
        reset = torch.cat([torch.zeros_like(d[:1]), d[:-1]], 0)
        outs = {}
        for name, dt in (("64", torch.float64), ("32", torch.float32)):
            m = copy.deepcopy(pol).to(dt)
            with torch.no_grad():
                outs[name] = m.unroll(c["observations"].to(dt), c["privileged_observations"].to(dt), (c["h_a"][0].to(dt), c["c_a"][0].to(dt)),
                                      (c["h_c"][0].to(dt), c["c_c"][0].to(dt)), reset)
        for k, got, i in (("mu", c["mu"], 0), ("values", c["values"], 1)):
            ok, line = rh.bound_check(f"iteration {it} {k}", got.numpy(), outs["64"][i].numpy(), outs["32"][i].numpy())
            if not ok:
                bad.append(line)
    assert not bad, "\n".join([rh.BOUND_HEADER] + bad)


def test_captured_replay_equals_the_eager_loop(two_iterations):
    import torch

    _, snaps, _, _ = two_iterations
    env, pol, st, rec, col = _setup(True)
    for it in range(4):  # iteration 0 is eager, 1 is the capture and its first replay, 2 and 3 are replays
        col.collect()
        got = _snapshot(st, rec)
        if it < 2:
            for k, v in snaps[it].items():
                assert torch.equal(got[k].view(torch.uint8), v.view(torch.uint8)), f"iteration {it}: {k} differs between the graphed and the eager collector"
        assert bool(torch.isfinite(got["returns"]).all())
    assert col._graph is not None
    # ... and against an eager collector that ran as long
    env2, _, st2, rec2, col2 = _setup(False)
    for it in range(4):
        col2.collect()
    want = _snapshot(st2, rec2)
    for k, v in want.items():
        assert torch.equal(got[k].view(torch.uint8), v.view(torch.uint8)), f"iteration 3 (second replay): {k} differs from the eager loop"
    for x in (rec, st, env, rec2, st2, env2):
        x.close()


# ---- Trainer and runner --------------------------------------------------------------------------------------------------------------
def test_ten_iterations_move_every_parameter():
    """A1 Flat, 512 envs x 24 steps (the size of tests/test_gpu_obsnorm_symmetry_train.py's ten-iteration run), H = 256 in front of 128-128-128 heads;
    one epoch per update keeps the torch BPTT of the test short"""
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    n = 512
    env = ManagerBasedRLEnv(FLAT, num_envs=n, seed=42, device=DEV)
    tr = Trainer(env, seed=42, rnn_type="lstm", rnn_hidden_dim=256, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128), num_learning_epochs=1)
    env.episode_length_buf = torch.randint(0, env.max_episode_length, (n,), generator=torch.Generator().manual_seed(0))
    before = {k: v.clone() for k, v in tr.state_dict().items()}
    assert "recurrent=lstm(256)" in repr(tr)
    for _ in range(10):
        out = tr.iterate()
        assert all(np.isfinite(out[k]) for k in ("value_loss", "surrogate_loss", "entropy", "kl", "learning_rate", "mean_reward", "action_std")), out
    after = tr.state_dict()
    for k in before:
        assert bool(torch.isfinite(after[k]).all()) and not torch.equal(before[k], after[k]), f"{k} did not move"
    assert {f"memory_{m}.rnn.{w}_l0" for m in "ac" for w in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")} <= set(after)
    # the collection runs the pushed parameters: the cell's image against the module, through one step
    x = torch.randn(n, tr.recurrent.cell_a.in_dim, device=DEV)
    z = torch.zeros(n, 256, device=DEV)
    h1, c1 = torch.empty_like(z), torch.empty_like(z)
    tr.recurrent.cell_a.step(x, z, z.clone(), h1, c1)
    with torch.no_grad():
        want, _ = tr.policy.memory_a(x.unsqueeze(0), z, z)
    torch.testing.assert_close(h1, want[0], rtol=0, atol=2e-6)
    tr.recurrent.close(); tr.storage.close(); env.close()


def _runner(cfg, n=64):
    from robot_lab_amd import shims

    shims.install()
    import gymnasium as gym
    from isaaclab_rl.rsl_rl import RslRlVecEnvWrapper
    from rsl_rl.runners import OnPolicyRunner

    gym.register(id=FLAT, entry_point="isaaclab.envs:ManagerBasedRLEnv", disable_env_checker=True, kwargs={})
    env = RslRlVecEnvWrapper(gym.make(FLAT, cfg=FLAT, num_envs=n, seed=3, device=DEV), clip_actions=None)
    return env, OnPolicyRunner(env, dict(cfg, seed=7, num_steps_per_env=24, save_interval=100), log_dir=None, device=DEV)


def test_checkpoint_round_trip_and_both_spellings(tmp_path):
    import torch

    cfg = copy.deepcopy(RSL_RL_SPELLING)
    cfg["algorithm"].update(num_learning_epochs=2, num_mini_batches=4)
    env_a, a = _runner(cfg)
    a.learn(num_learning_iterations=2)
    path = str(tmp_path / "model.pt")
    a.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=False)["model_state_dict"]
    assert {"memory_a.rnn.weight_ih_l0", "memory_a.rnn.weight_hh_l0", "memory_a.rnn.bias_ih_l0", "memory_a.rnn.bias_hh_l0", "memory_c.rnn.weight_ih_l0",
            "actor.0.weight", "critic.6.bias", "std"} <= set(sd)
    ref_cfg = copy.deepcopy(REFERENCE_SPELLING)
    ref_cfg["algorithm"].update(num_learning_epochs=2, num_mini_batches=4)
    env_b, b = _runner(ref_cfg)  # the reference's spelling builds the same module shapes
    assert {k: tuple(v.shape) for k, v in b.alg.policy.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert b.load(path) is None and b.current_learning_iteration == 2
    for (k, p), q in zip(a.alg.policy.state_dict().items(), b.alg.policy.state_dict().values()):
        assert torch.equal(p, q), k
    # one more update on a shared batch: bit-identical parameters
    batch = a.trainer.update_batch()
    a.alg.update(batch)
    b.alg.update(batch)
    for (k, p), q in zip(a.alg.policy.state_dict().items(), b.alg.policy.state_dict().values()):
        assert torch.equal(p, q), f"{k} differs after one more update from the checkpoint"
    # the inference policy is stateful and `reset(dones)` is what play.py:246 calls
    policy = b.get_inference_policy(device=DEV)
    obs = env_b.get_observations()
    with torch.inference_mode():
        first = policy(obs).clone()
        again = policy(obs).clone()  # same observation, advanced memory
        assert not torch.equal(first, again)
        dones = torch.zeros(64, dtype=torch.bool, device=DEV)
        dones[::2] = True
        b.alg.policy.reset(dones)
        third = policy(obs).clone()
        assert torch.equal(third[::2], first[::2]) and not torch.equal(third[1::2], first[1::2])  # a reset row starts over, bit for bit
        policy.reset()
        assert torch.equal(policy(obs), first)
        for _ in range(3):
            obs, _, dones, _ = env_b.step(policy(obs))
            b.alg.policy.reset(dones)
    env_a.close(); env_b.close()


def test_device_side_refusals():
    import torch

    from robot_lab_amd.collect import Collector
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.lstm import LstmCell, RecurrentState
    from robot_lab_amd.ppo import Trainer

    env, pol, st, rec, col = _setup(False)
    for kw, reason in ((dict(overlap=True), "overlap=True"), (dict(fused_act=True), "fused_act"), (dict(normalizers=(object(), None)), "normalizers")):
        with pytest.raises(NotImplementedError, match=reason):
            Collector(env, col.actor, col.critic, st, col.std, recurrent=rec, **kw)
    small = RecurrentState(rec.cell_a, rec.cell_c, N // 2, T)
    with pytest.raises(ValueError, match="sized"):
        Collector(env, col.actor, col.critic, st, col.std, recurrent=small)
    with pytest.raises(ValueError, match="MLP heads"):
        Collector(env, col.critic, col.actor, st, col.std, recurrent=RecurrentState(rec.cell_a, LstmCell(*rh.lstm_default_init(7, 20, 0), device=DEV), N, T))
    assert col.fused_act is False and col.use_graph is False
    x = torch.zeros(N, rec.cell_a.in_dim, device=DEV)
    (ha, ca), _ = rec.state()
    with pytest.raises(ValueError, match="aliases"):
        rec.cell_a.step(x, ha, ca, ha, ca)
    with pytest.raises(ValueError, match="float32"):
        rec.cell_a.step(x.double(), ha, ca, torch.empty_like(ha), torch.empty_like(ca))
    for kw, reason in ((dict(learner="hip"), "back-propagation through time"), (dict(rnn_type="gru"), "gru"), (dict(rnn_num_layers=2), "rnn_num_layers"),
                       (dict(symmetry="lr"), "symmetry"), (dict(actor_obs_normalization=True), "normalisation")):
        with pytest.raises(NotImplementedError, match=reason):
            Trainer(env, **{"rnn_type": "lstm", **kw})
    rec.close(); st.close(); env.close()
