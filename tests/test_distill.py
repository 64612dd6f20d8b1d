"""CPU tier of the distillation rule (robot_lab_amd/distill.py), the cfg containers and the runner's cfg reader: the grouping of
`Distillation.update` across epochs, its gradient on an exact integer family (with teeth: four defects that must not reproduce it),
`StudentTeacher.load_state_dict`, the reference's distillation cfg through the shims, and every refusal of the runner.  The HIP learner's
numerics are tests/test_gpu_distill.py."""
import copy
import os

import numpy as np
import pytest
import torch

from distill_helpers import EX, exact_family, exact_group_gradient, exact_policy, recorded_update
from robot_lab_amd import shims
from robot_lab_amd.distill import Distillation, StudentTeacher, update_groups
from robot_lab_amd.ppo import ActorCritic

REF = "/root/reference/source/robot_lab"
shims.install()
GROUPS = [(0, 1, 2), (3, 4, 0), (1, 2, 3)]


def test_groups_run_across_the_epochs():
    groups, left = update_groups(5, 3, 2)
    assert groups == GROUPS and left == (4,)
    assert update_groups(4, 2, 2) == ([(0, 1), (2, 3), (0, 1), (2, 3)], ())
    assert update_groups(2, 5, 2) == ([], (0, 1, 0, 1))


@pytest.mark.parametrize("loss_type", ["mse", "huber"])
def test_update_is_three_steps_over_the_listed_groups_and_the_left_over_only_counts(loss_type):
    torch.manual_seed(0)
    pol = StudentTeacher(10, 10, 3, student_hidden=(16,), teacher_hidden=(8,))
    g = torch.Generator().manual_seed(1)
    import types

    batch = types.SimpleNamespace(observations=torch.randn(5, 7, 10, generator=g), teacher_actions=2.0 * torch.randn(5, 7, 3, generator=g))
    twin = copy.deepcopy(pol)
    teacher_before = copy.deepcopy(pol.teacher.state_dict())
    alg = Distillation(pol, num_learning_epochs=2, gradient_length=3, learning_rate=1e-2, loss_type=loss_type)
    res, grads, params = recorded_update(alg, batch)
    assert len(grads) == 3 and alg.num_updates == 3
    # the same thing written out: the listed groups, then step 4 of the second epoch for the statistic alone
    fn = torch.nn.functional.mse_loss if loss_type == "mse" else torch.nn.functional.huber_loss
    opt = torch.optim.Adam(twin.parameters(), lr=1e-2)
    losses = []
    for steps in GROUPS:
        ls = [fn(twin.student(batch.observations[t]), batch.teacher_actions[t]) for t in steps]
        losses += [float(l.detach()) for l in ls]
        opt.zero_grad()
        sum(ls[1:], ls[0]).backward()
        opt.step()
    with torch.no_grad():
        losses.append(float(fn(twin.student(batch.observations[4]), batch.teacher_actions[4])))
    assert len(losses) == 10  # cnt
    for a, b in zip(pol.student.parameters(), twin.student.parameters()):
        assert torch.equal(a, b)
    after = torch.cat([p.detach().reshape(-1) for p in pol.student.parameters()]).double()
    assert torch.equal(after, params[2])  # nothing moved after the third step: the left-over changes no parameter ...
    assert res["behavior"] == sum(losses) / 10  # ... but counts in the mean
    for k, v in pol.teacher.state_dict().items():
        assert torch.equal(v, teacher_before[k])
    assert float(pol.std[0]) == pytest.approx(0.1) and pol.std.grad is None


def test_exact_family_gradient_is_the_int64_result_bit_for_bit_and_defects_are_not():
    pol, batch = exact_policy()
    alg = Distillation(pol, num_learning_epochs=EX["epochs"], gradient_length=EX["gradient_length"], learning_rate=1e-3)
    res, grads, _ = recorded_update(alg, batch, step=False)  # frozen parameters: every group's gradient at the integer weights
    want = [exact_group_gradient(s) for s in GROUPS]
    assert len(grads) == 3
    for g, w in zip(grads, want):
        assert np.array_equal(g.numpy().astype(np.float32), w) and np.array_equal(g.numpy(), w.astype(np.float64))
    got = np.stack([g.numpy() for g in grads])
    # the defects: none of them reproduces the rule's gradients
    third = np.stack([w.astype(np.float64) / 3.0 for w in want])                       # a scale of 1 / (gradient_length N A)
    restart = [exact_group_gradient(s).astype(np.float64) for s in [(0, 1, 2), (3, 4), (0, 1, 2)]]  # groups that restart at the epoch boundary
    leftover = exact_group_gradient((1, 2, 3, 4)).astype(np.float64)                    # a left-over that is back-propagated (with the last group)
    half = np.stack([exact_group_gradient(s, shift=-10).astype(np.float64) for s in GROUPS])  # a missing factor 2
    assert not np.array_equal(third, got)
    assert not np.array_equal(restart[1], got[1]) and not np.array_equal(restart[2], got[2])
    assert not np.array_equal(leftover, got[2]) and not np.array_equal(exact_group_gradient((4,)).astype(np.float64), np.zeros_like(got[2]))
    assert not np.array_equal(half, got)
    # behavior: the mean of the ten per-step losses, each exact (sum d^2 < 2^24 ... / 2^10)
    W, obs, ta = exact_family()
    per_step = [float(np.float32(((obs[t] @ W.T - ta[t]) ** 2).sum() / 1024.0)) for t in [0, 1, 2, 3, 4] * 2]
    assert res["behavior"] == pytest.approx(sum(per_step) / 10, rel=1e-6)


# ---- StudentTeacher.load_state_dict
def test_state_dict_keys_are_rsl_rls():
    pol = StudentTeacher(10, 14, 3, student_hidden=(16, 16), teacher_hidden=(32,), teacher_obs_normalization=True)
    assert list(pol.state_dict().keys()) == ["std", "student.0.weight", "student.0.bias", "student.2.weight", "student.2.bias", "student.4.weight",
                                             "student.4.bias", "teacher.0.weight", "teacher.0.bias", "teacher.2.weight", "teacher.2.bias",
                                             "teacher_obs_normalizer._mean", "teacher_obs_normalizer._var", "teacher_obs_normalizer._std",
                                             "teacher_obs_normalizer.count"]
    assert [n for n, _ in pol.named_children()][:2] == ["student", "teacher"]
    assert not pol.teacher.training and all(not p.requires_grad for p in pol.teacher.parameters())
    pol.train()
    assert not pol.teacher.training and not pol.teacher_obs_normalizer.training


def test_ppo_checkpoint_fills_the_teacher_and_is_not_a_resume():
    torch.manual_seed(1)
    ppo = ActorCritic(14, 20, 3, actor_hidden=(32,), critic_hidden=(8,))
    pol = StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,))
    student = copy.deepcopy(pol.student.state_dict())
    assert not pol.loaded_teacher
    assert pol.load_state_dict(ppo.state_dict()) is False and pol.loaded_teacher
    for k, v in ppo.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k], v)
    for k, v in student.items():
        assert torch.equal(pol.student.state_dict()[k], v)
    x = torch.randn(5, 14)
    assert torch.equal(pol.evaluate(x), ppo.actor(x)) and not pol.evaluate(x).requires_grad
    with pytest.raises(RuntimeError):  # strict on shapes
        StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(64,)).load_state_dict(ppo.state_dict())


def test_ppo_checkpoint_with_a_normaliser():
    torch.manual_seed(2)
    ppo = ActorCritic(14, 20, 3, actor_hidden=(32,), critic_hidden=(8,), actor_obs_normalization=True)
    ppo.actor_obs_normalizer.update(3.0 + 2.0 * torch.randn(50, 14))
    pol = StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,), teacher_obs_normalization=True)
    assert pol.load_state_dict(ppo.state_dict()) is False
    for k, v in ppo.actor_obs_normalizer.state_dict().items():
        assert torch.equal(pol.teacher_obs_normalizer.state_dict()[k], v)
    x = torch.randn(5, 14)
    assert torch.equal(pol.evaluate(x), ppo.actor(ppo.actor_obs_normalizer(x)))
    before = copy.deepcopy(pol.teacher_obs_normalizer.state_dict())
    pol.train()
    pol.teacher_obs_normalizer.update(torch.randn(9, 14))  # applied, never updated
    for k, v in before.items():
        assert torch.equal(pol.teacher_obs_normalizer.state_dict()[k], v)
    with pytest.raises(RuntimeError, match="teacher_obs_normalization"):  # a normaliser on one side only, either side
        StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,)).load_state_dict(ppo.state_dict())
    plain = ActorCritic(14, 20, 3, actor_hidden=(32,), critic_hidden=(8,))
    with pytest.raises(RuntimeError, match="teacher_obs_normalization"):
        StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,), teacher_obs_normalization=True).load_state_dict(plain.state_dict())


def test_distillation_checkpoint_resumes_and_anything_else_is_an_error():
    torch.manual_seed(3)
    a = StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,))
    b = StudentTeacher(10, 14, 3, student_hidden=(16,), teacher_hidden=(32,))
    assert b.load_state_dict(a.state_dict()) is True and b.loaded_teacher
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v)
    with pytest.raises(ValueError, match="neither"):
        b.load_state_dict({"critic.0.weight": torch.zeros(1)})
    with pytest.raises(RuntimeError):  # strict
        b.load_state_dict({k: v for k, v in a.state_dict().items() if k != "std"})


# ---- cfg containers and the runner's cfg reader
def _cfg(**over):
    shims.install()
    from isaaclab_rl.rsl_rl import RslRlDistillationAlgorithmCfg, RslRlDistillationRunnerCfg, RslRlMLPModelCfg

    model = lambda std: RslRlMLPModelCfg(hidden_dims=[128, 128, 128], activation="elu", obs_normalization=False,  # noqa: E731
                                         distribution_cfg=RslRlMLPModelCfg.GaussianDistributionCfg(init_std=std))
    cfg = RslRlDistillationRunnerCfg(num_steps_per_env=120, max_iterations=3, save_interval=50, experiment_name="x",
                                     obs_groups={"student": ["policy"], "teacher": ["policy"]}, student=model(0.1), teacher=model(0.0),
                                     algorithm=RslRlDistillationAlgorithmCfg(num_learning_epochs=2, learning_rate=1e-3, gradient_length=15))
    d = cfg.to_dict()
    for path, v in over.items():
        node, keys = d, path.split("__")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = v
    return d


def _check_reference_numbers(kw):
    assert kw["student_hidden"] == (128, 128, 128) and kw["teacher_hidden"] == (128, 128, 128) and kw["init_noise_std"] == 0.1
    assert kw["num_learning_epochs"] == 2 and kw["learning_rate"] == 1e-3 and kw["gradient_length"] == 15 and kw["num_steps_per_env"] == 120
    assert kw["student_group"] == "policy" and kw["teacher_group"] == "policy"
    assert kw["max_grad_norm"] is None and kw["loss_type"] == "mse" and kw["teacher_obs_normalization"] is False


def test_cfg_containers_carry_class_names_and_the_reader_gets_the_numbers():
    from rsl_rl.runners import read_distillation_cfg

    d = _cfg()
    assert d["class_name"] == "DistillationRunner" and d["algorithm"]["class_name"] == "Distillation"
    assert d["student"]["class_name"] == "MLPModel" and d["student"]["distribution_cfg"]["init_std"] == 0.1
    _check_reference_numbers(read_distillation_cfg(d))
    import isaaclab_rl.rsl_rl as m

    assert m.RslRlSymmetryCfg.__mro__[1].__name__ == "GenericCfg"  # the generic fallback stays for everything else


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's cfg file")
def test_reference_distillation_cfg_imports_unchanged_and_reads():
    shims.install(shims.REFERENCE_SOURCE)
    import importlib

    from rsl_rl.runners import read_distillation_cfg

    mod = importlib.import_module("robot_lab.tasks.manager_based.locomotion.velocity.config.quadruped.anymal_d.agents.rsl_rl_distillation_cfg")
    d = mod.AnymalDFlatDistillationRunnerCfg().to_dict()
    assert d["class_name"] == "DistillationRunner"
    _check_reference_numbers(read_distillation_cfg(d))
    with pytest.raises(NotImplementedError, match="rnn_type"):
        read_distillation_cfg(mod.AnymalDFlatDistillationRunnerRecurrentCfg().to_dict())


@pytest.mark.parametrize("over, error, match", [
    (dict(student__rnn_type="lstm"), NotImplementedError, "rnn_type"),
    (dict(teacher__rnn_type="gru"), NotImplementedError, "rnn_type"),
    (dict(student__obs_normalization=True), NotImplementedError, "student obs_normalization"),
    (dict(algorithm__optimizer="sgd"), NotImplementedError, "optimizer='sgd'"),
    (dict(student__activation="relu"), NotImplementedError, "activation='relu'"),
    (dict(teacher__activation="tanh"), NotImplementedError, "activation='tanh'"),
    (dict(obs_groups={"student": ["policy", "critic"], "teacher": ["policy"]}), NotImplementedError, "exactly one observation group"),
    (dict(obs_groups={"student": ["policy"], "teacher": ["privileged"]}), ValueError, "no observation group 'privileged'"),
    (dict(policy=dict(class_name="StudentTeacher", student_hidden_dims=[128])), NotImplementedError, "`student` / `teacher`"),
])
def test_runner_refuses_with_a_reason(over, error, match):
    from rsl_rl.runners import read_distillation_cfg

    with pytest.raises(error, match=match):
        read_distillation_cfg(_cfg(**over))


def test_runner_refuses_more_than_one_rank_before_anything_else(monkeypatch):
    shims.install()
    from rsl_rl.runners import DistillationRunner

    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="2 ranks"):
        DistillationRunner(None, _cfg())


def test_critic_group_is_accepted_for_either_network():
    from rsl_rl.runners import read_distillation_cfg

    kw = read_distillation_cfg(_cfg(obs_groups={"student": ["policy"], "teacher": ["critic"]}, teacher__obs_normalization=True, algorithm__max_grad_norm=0.5,
                                    algorithm__loss_type="huber"))
    assert kw["teacher_group"] == "critic" and kw["teacher_obs_normalization"] is True and kw["max_grad_norm"] == 0.5 and kw["loss_type"] == "huber"
