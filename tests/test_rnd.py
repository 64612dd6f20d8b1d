"""CPU tier of random network distillation: the torch rule (robot_lab_amd/rnd.py) against an independent numpy restatement in fp64, the invariants of
the update (the target never moves, the PPO half does not notice), the teeth of the GPU tier's bound, and the cfg reading with every refusal.
The device halves are tests/test_rnd_abi.py (no device) and tests/test_gpu_rnd.py."""
import copy
import types

import numpy as np
import pytest
import torch

from ppo_helpers import fake_storage
from rnd_helpers import WRONG_RULES, NpRnd, bound_ratio, cast_layers, make_layers, module_from_layers, module_tensors
from robot_lab_amd.ppo import PPO, ActorCritic
from robot_lab_amd.rnd import RandomNetworkDistillation, check_rnd, make_optimizer, read_rnd_cfg, read_schedule, schedule_weight, update_minibatch

T, N, S, K = 6, 5, 7, 3
EPOCHS, MINI_BATCHES = 2, 2
SCHEDULES = {"constant": None, "step": dict(mode="step", final_step=4, final_value=0.25),
             "linear": dict(mode="linear", initial_step=2, final_step=5, final_value=3.0)}


def _case(seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    pred, targ = make_layers(rng, [S, 16, 8, K]), make_layers(rng, [S, 12, K], scale=scale)
    states = rng.standard_normal((T + 1, N, S)) * np.linspace(0.5, 2.0, S) + 0.3  # (per-column scales: the normaliser has something to do)
    slots = rng.standard_normal((T, N))
    perm = rng.permutation(T * N)
    return pred, targ, states, slots, perm


def _run_numpy(pred, targ, states, slots, perm, dtype, wrong=None, schedule=None, norm=True):
    ref = NpRnd(cast_layers(pred, dtype), cast_layers(targ, dtype), weight=0.7, schedule=schedule, state_normalization=norm, reward_normalization=norm, wrong=wrong)
    slots = slots.astype(dtype).copy()
    rewards = np.stack([ref.collect_step(slots[t], states[t + 1]) for t in range(T)])
    loss = ref.update(states[:T].reshape(T * N, S), perm, EPOCHS, MINI_BATCHES)
    return ref, rewards, slots, loss


def _run_torch(pred, targ, states, slots, perm, dtype, schedule=None, norm=True):
    m = module_from_layers(pred, targ, dtype, weight=0.7, weight_schedule=schedule, state_normalization=norm, reward_normalization=norm)
    slots_t = torch.as_tensor(slots).to(dtype).clone()
    rewards = torch.stack([m.collect_step(slots_t[t], torch.as_tensor(states[t + 1]).to(dtype)) for t in range(T)])
    opt = make_optimizer(m)
    rows = torch.as_tensor(states[:T].reshape(T * N, S)).to(dtype)
    mb = len(perm) // MINI_BATCHES
    losses = [update_minibatch(m, opt, rows[torch.as_tensor(perm[i * mb:(i + 1) * mb])]) for _ in range(EPOCHS) for i in range(MINI_BATCHES)]
    return m, opt, rewards.numpy(), slots_t.numpy(), float(np.mean(losses))


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_the_rule_agrees_with_the_numpy_restatement_in_fp64(schedule):
    case = _case()
    ref, r_np, slots_np, loss_np = _run_numpy(*case, np.float64, schedule=SCHEDULES[schedule])
    m, opt, r_t, slots_t, loss_t = _run_torch(*case, torch.float64, schedule=SCHEDULES[schedule])
    np.testing.assert_allclose(r_t, r_np, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(slots_t, slots_np, rtol=1e-10, atol=1e-10)
    assert abs(loss_t - loss_np) <= 1e-10 * max(1.0, abs(loss_np))
    assert m.update_counter == ref.count == T
    for a, b in ((m.state_normalizer._mean, ref.snorm.mean), (m.state_normalizer._std, ref.snorm.std), (m.reward_normalizer.emp_norm._std, ref.rnorm.std),
                 (m.reward_normalizer.avg, ref.avg)):
        np.testing.assert_allclose(a.numpy().reshape(-1), np.asarray(b).reshape(-1), rtol=1e-10, atol=1e-10)
    got, want = module_tensors(m, opt), ref.tensors()
    assert set(got) == set(want)
    for name in want:
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=1e-10, err_msg=name)
    if schedule != "constant":  # the weight moved inside the window
        assert m.weight != 0.7 and m.weight == SCHEDULES[schedule]["final_value"]


def test_the_schedules():
    assert [schedule_weight(2.0, *read_schedule(None), c) for c in (1, 100)] == [2.0, 2.0]
    assert [schedule_weight(2.0, *read_schedule("constant"), c) for c in (1, 100)] == [2.0, 2.0]
    step = read_schedule(dict(mode="step", final_step=10, final_value=0.5))
    assert [schedule_weight(2.0, *step, c) for c in (1, 9, 10, 11)] == [2.0, 2.0, 0.5, 0.5]
    lin = read_schedule(dict(mode="linear", initial_step=10, final_step=20, final_value=4.0))
    assert [schedule_weight(2.0, *lin, c) for c in (1, 10, 15, 20, 99)] == [2.0, 2.0, 3.0, 4.0, 4.0]
    for bad in ("cosine", dict(mode="cosine"), "step", dict(mode="step", final_step=3), dict(mode="linear", initial_step=5, final_step=5, final_value=1.0)):
        with pytest.raises(ValueError, match="weight_schedule"):
            read_schedule(bad)


def test_state_dict_keys_and_the_target_is_bit_identical_after_an_update():
    pred, targ, states, slots, perm = _case()
    m, opt, *_ = _run_torch(pred, targ, states, slots, perm, torch.float32)
    keys = set(m.state_dict())
    assert {k.split(".")[0] for k in keys} == {"predictor", "target", "state_normalizer", "reward_normalizer"}
    assert {"state_normalizer._mean", "state_normalizer.count", "reward_normalizer.emp_norm._std", "predictor.0.weight", "target.2.bias"} <= keys
    lin = [x for x in m.target if isinstance(x, torch.nn.Linear)]
    for x, (w, b) in zip(lin, cast_layers(targ, np.float32)):
        assert np.array_equal(x.weight.detach().numpy().view(np.int32), w.view(np.int32)) and np.array_equal(x.bias.detach().numpy().view(np.int32), b.view(np.int32))
    assert all(p.grad is None for p in m.target.parameters())
    moved = [x for x in m.predictor if isinstance(x, torch.nn.Linear)][0].weight.detach().numpy()
    assert not np.array_equal(moved, cast_layers(pred, np.float32)[0][0])


@pytest.mark.parametrize("group", ["policy", "critic"])
def test_the_ppo_half_is_bit_identical_with_and_without_rnd(group):
    torch.manual_seed(0)
    pol = ActorCritic(10, 14, 3, actor_hidden=(32, 16), critic_hidden=(32, 16))
    st = fake_storage(pol, T=4, N=16)
    rnd = RandomNetworkDistillation(10 if group == "policy" else 14, num_outputs=K, predictor_hidden_dims=(16,), target_hidden_dims=(8,), weight=1.0,
                                    state_normalization=True, group=group)
    rnd.state_normalizer.update(st.observations.reshape(-1, 10) if group == "policy" else st.privileged_observations.reshape(-1, 14))
    before = copy.deepcopy(rnd.state_dict())
    algs = [PPO(copy.deepcopy(pol), num_learning_epochs=2, num_mini_batches=2), PPO(copy.deepcopy(pol), num_learning_epochs=2, num_mini_batches=2, rnd=rnd)]
    outs = [alg.update(st, torch.Generator().manual_seed(3)) for alg in algs]
    for a, b in zip(algs[0].policy.parameters(), algs[1].policy.parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    assert set(outs[1]) - set(outs[0]) == {"rnd_loss"} and outs[1]["rnd_loss"] > 0
    assert {k: v for k, v in outs[1].items() if k != "rnd_loss"} == outs[0]
    assert list(outs[1])[-1] == "learning_rate"
    after = rnd.state_dict()
    for k in before:
        assert torch.equal(before[k], after[k]) == (not k.startswith("predictor.")), k
    # ... and the RND half is update_minibatch on the rows of the same permutation
    ref = RandomNetworkDistillation(rnd.state_dim, num_outputs=K, predictor_hidden_dims=(16,), target_hidden_dims=(8,), weight=1.0, state_normalization=True, group=group)
    ref.load_state_dict(before)
    opt, rows = make_optimizer(ref), (st.observations if group == "policy" else st.privileged_observations).reshape(64, -1)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(3))
    losses = [update_minibatch(ref, opt, rows[perm[i * 32:(i + 1) * 32]]) for _ in range(2) for i in range(2)]
    assert outs[1]["rnd_loss"] == pytest.approx(float(np.mean(losses)), rel=1e-12)
    for a, b in zip(ref.predictor.parameters(), rnd.predictor.parameters()):
        assert torch.equal(a, b)


# ---- teeth: every wrong rule misses the bound the GPU tier holds the kernels to (e <= 8 d, d the fp32 rule's own distance from fp64) -------------
@pytest.mark.parametrize("wrong", WRONG_RULES)
def test_a_wrong_rule_misses_the_gpu_bound(wrong):
    case = _case(scale=40.0)  # (a far target: the gradient norm is above 1, so a clipped gradient is a different gradient)
    ref64, r64, _, _ = _run_numpy(*case, np.float64)
    ref32, r32, _, _ = _run_numpy(*case, np.float32)
    bad, rb, _, _ = _run_numpy(*case, np.float64, wrong=wrong)
    if wrong == "clipped_grad":
        norm = np.sqrt(sum(float((g ** 2).sum()) for pair in _run_numpy(*case, np.float64)[0].last_grads for g in pair))
        assert norm > 1.5, norm
    worst_name, worst = "intrinsic reward", bound_ratio(rb, r64, r32)
    t64, t32, tb = ref64.tensors(), ref32.tensors(), bad.tensors()
    for name in t64:
        ratio = bound_ratio(tb[name], t64[name], t32[name])
        if ratio[2] > worst[2]:
            worst_name, worst = name, ratio
    print(f"wrong rule {wrong:<14} misses the bound by a factor {worst[2]:.3g} on {worst_name} (e {worst[0]:.3e}, d {worst[1]:.3e})")
    assert worst[2] > 1.0, (wrong, worst_name, worst)
    where = "intrinsic reward" if wrong in ("squared_norm", "std_before", "no_discount") else "update"
    if where == "intrinsic reward":
        assert bound_ratio(rb, r64, r32)[2] > 1.0
    else:  # the collection is untouched by a wrong update
        assert np.array_equal(rb, r64)


def test_the_right_rule_in_fp32_is_inside_its_own_bound():
    case = _case(scale=40.0)
    ref64, r64, _, _ = _run_numpy(*case, np.float64)
    m, opt, r_t, _, _ = _run_torch(*case, torch.float32)
    _, r32, _, _ = _run_numpy(*case, np.float32)
    assert bound_ratio(r_t, r64, r32)[2] <= 1.0
    t64, t32, got = ref64.tensors(), _run_numpy(*case, np.float32)[0].tensors(), module_tensors(m, opt)
    for name in t64:
        assert bound_ratio(got[name], t64[name], t32[name])[2] <= 1.0, name


# ---- cfg reading ---------------------------------------------------------------------------------------------------------------------------
RND_CFG = dict(weight=0.5, weight_schedule=dict(mode="step", final_step=100, final_value=0.1), reward_normalization=True, state_normalization=True,
               learning_rate=2e-3, num_outputs=4, predictor_hidden_dims=[64, 32], target_hidden_dims=[48])
TRAIN_CFG = dict(num_steps_per_env=4, seed=1, policy=dict(class_name="ActorCritic", actor_hidden_dims=[32], critic_hidden_dims=[32], activation="elu", init_noise_std=1.0),
                 algorithm=dict(class_name="PPO", num_learning_epochs=2, num_mini_batches=2, rnd_cfg=RND_CFG))


def test_cfg_reading_both_spellings_of_obs_groups():
    want = dict(RND_CFG, predictor_hidden_dims=(64, 32), target_hidden_dims=(48,), group="policy")
    assert read_rnd_cfg(TRAIN_CFG) == want
    assert read_rnd_cfg(dict(TRAIN_CFG, obs_groups={"policy": ["policy"], "critic": ["critic"], "rnd_state": ["critic"]})) == dict(want, group="critic")
    assert read_rnd_cfg(dict(TRAIN_CFG, obs_groups={"actor": ["policy"], "critic": ["critic"], "rnd_state": ["policy"]})) == want
    assert read_rnd_cfg(dict(TRAIN_CFG, algorithm={})) is None and read_rnd_cfg({}) is None
    with pytest.raises(NotImplementedError, match="ONE observation group"):
        read_rnd_cfg(dict(TRAIN_CFG, obs_groups={"rnd_state": ["policy", "critic"]}))
    with pytest.raises(NotImplementedError, match="-1"):  # IsaacLab's defaults
        read_rnd_cfg(dict(TRAIN_CFG, algorithm=dict(rnd_cfg=dict(weight=1.0))))


def test_the_shim_cfg_class_has_isaaclabs_fields():
    from robot_lab_amd import shims

    shims.install()
    from isaaclab_rl.rsl_rl import RslRlRndCfg

    cfg = RslRlRndCfg(weight=0.5, predictor_hidden_dims=[64, 32], target_hidden_dims=[48], weight_schedule=RslRlRndCfg.LinearWeightScheduleCfg(final_value=0.1, initial_step=10, final_step=20))
    d = cfg.to_dict()
    assert set(d) == {"weight", "weight_schedule", "reward_normalization", "state_normalization", "learning_rate", "num_outputs", "predictor_hidden_dims", "target_hidden_dims"}
    got = read_rnd_cfg(dict(algorithm=dict(rnd_cfg=d)))
    assert got["weight"] == 0.5 and got["weight_schedule"]["mode"] == "linear" and got["num_outputs"] == 1 and got["learning_rate"] == 1e-3


class NoEnv:
    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the refusal")


def test_trainer_refusals_come_before_the_env_is_touched():
    from robot_lab_amd.ppo import Trainer

    rnd = dict(weight=1.0, predictor_hidden_dims=[8], target_hidden_dims=[8])
    group = type("G", (), {"world_size": 2})()
    for kw, exc, reason in ((dict(rnn_type="lstm"), NotImplementedError, "rnd= with rnn_type"), (dict(symmetry="lr"), NotImplementedError, "rnd= with symmetry"),
                            (dict(mirror_loss=0.5), NotImplementedError, "rnd= with symmetry"),
                            (dict(actor_obs_normalization=True), NotImplementedError, "rnd= with actor_obs_normalization"),
                            (dict(critic_obs_normalization=True), NotImplementedError, "rnd= with actor_obs_normalization"),
                            (dict(group=group), NotImplementedError, "2 ranks"), (dict(learner="jax"), ValueError, "learner")):
        with pytest.raises(exc, match=reason):
            Trainer(NoEnv(), rnd=rnd, **kw)
    for bad, exc, reason in ((dict(rnd, predictor_hidden_dims=[-1]), NotImplementedError, "-1"), (dict(rnd, target_hidden_dims=[64, -1]), NotImplementedError, "-1"),
                             (dict(rnd, group=["policy", "critic"]), NotImplementedError, "ONE observation group"), (dict(rnd, group="teacher"), ValueError, "group"),
                             (dict(rnd, num_outputs=0), ValueError, "num_outputs"), (dict(rnd, learning_rate=0.0), ValueError, "learning_rate"),
                             (dict(rnd, weight=float("nan")), ValueError, "weight"), (dict(rnd, bonus=1), ValueError, "unknown keys"),
                             (dict(rnd, predictor_hidden_dims=[1024]), ValueError, "width"), ("yes", TypeError, "dict")):
        with pytest.raises(exc, match=reason):
            Trainer(NoEnv(), rnd=bad)


def test_a_state_group_wider_than_512_is_refused_before_anything_is_built():
    from robot_lab_amd.ppo import Trainer

    class WideEnv:
        num_envs, num_actions = 4, 3

        def reset(self):
            return {"policy": torch.zeros(4, 45), "critic": torch.zeros(4, 600)}, {}

    with pytest.raises(ValueError, match="rnd state group 'critic' is 600 columns"):
        Trainer(WideEnv(), rnd=dict(weight=1.0, predictor_hidden_dims=[8], target_hidden_dims=[8], group="critic"))


def test_collector_refusals_need_no_device():
    from robot_lab_amd.collect import Collector

    with pytest.raises(NotImplementedError, match="overlap=True with rnd="):
        Collector(None, None, None, None, None, rnd=object(), overlap=True)
    for kw in (dict(recurrent=object()), dict(normalizers=(object(), None))):
        with pytest.raises(NotImplementedError, match="rnd= with recurrent= or normalizers="):
            Collector(None, None, None, None, None, rnd=object(), **kw)


def test_the_runner_builds_from_a_rnd_cfg_up_to_the_device(monkeypatch):
    """the stand-in runner no longer refuses `rnd_cfg`: it reads it and reaches the Trainer, which - on a stub env without a device - gets as far as the
    existing refusal tests do (the env's reset)"""
    from robot_lab_amd.shims.rsl_rl.runners import OnPolicyRunner

    monkeypatch.delenv("RL_LEARNER", raising=False)
    touched = []

    class StubEnv:
        clip_actions = None

        @property
        def unwrapped(self):
            return self

        def reset(self):
            touched.append("reset")
            raise RuntimeError("stub env: no device behind it")

    with pytest.raises(RuntimeError, match="stub env"):
        OnPolicyRunner(StubEnv(), TRAIN_CFG, device="cpu")
    assert touched == ["reset"]
    with pytest.raises(NotImplementedError, match="-1"):  # refused by the reader, the env untouched
        OnPolicyRunner(NoEnv(), dict(TRAIN_CFG, algorithm=dict(TRAIN_CFG["algorithm"], rnd_cfg=dict(weight=1.0))), device="cpu")
    with pytest.raises(NotImplementedError, match="ONE observation group"):
        OnPolicyRunner(NoEnv(), dict(TRAIN_CFG, obs_groups={"rnd_state": ["policy", "critic"]}), device="cpu")
    policy = dict(TRAIN_CFG["policy"], actor_obs_normalization=True)
    with pytest.raises(NotImplementedError, match="rnd= with actor_obs_normalization"):
        OnPolicyRunner(StubEnv(), dict(TRAIN_CFG, policy=policy), device="cpu")
    assert touched == ["reset"]


def test_check_rnd_fills_the_defaults():
    got = check_rnd("t", dict(weight=2, predictor_hidden_dims=[8], target_hidden_dims=(4, 4)))
    assert got == dict(weight=2.0, weight_schedule=None, reward_normalization=False, state_normalization=False, learning_rate=1e-3, num_outputs=1,
                       predictor_hidden_dims=(8,), target_hidden_dims=(4, 4), group="policy")
    assert isinstance(types.SimpleNamespace(**got).weight, float)
