"""CPU tier of recurrent distillation (robot_lab_amd/distill_recurrent.py): the torch rule against two independent definitions, the wrong rules it
must not be, checkpoints, the reference's cfg, the refusals.  The HIP learner's ABI is tests/test_distill_recurrent_abi.py, its numerics
tests/test_gpu_distill_recurrent.py.

Teeth, measured on the shape "wrap+left-over" (T 5, N 6, gradient length 3, 2 epochs; the largest max|wrong - rule| / max|rule| over every group's
gradient tensors, the final state and the final parameters, in fp64; the agreement asked of a right rule is 1e-10, and the largest multiple of d
over the tensors, where the GPU bound is 8):
    gradient crosses a done                           2.8e-01     1.3e+06 d
    gradient crosses a group boundary                 1.1e+00     3.1e+06 d
    gradient crosses an epoch boundary                3.3e-01     1.1e+06 d
    the epoch does not restart from h0                1.6e+00     4.6e+06 d
    the carried state is recomputed after the step    3.8e-03     4.1e+04 d
    the reset is applied one step late                8.8e-01     6.2e+06 d
    the left-over steps are back-propagated           2.9e-03     4.3e+04 d
    one bias gets no gradient                         1.0e+00     1.2e+07 d"""
import copy
import os

import numpy as np
import pytest
import torch

import distill_recurrent_helpers as dh
from distill_recurrent_helpers import DEFECTS, RULE_SHAPES
from robot_lab_amd import shims
from robot_lab_amd.distill_recurrent import RecurrentDistillation, StudentTeacherRecurrent
from robot_lab_amd.recurrent import ActorCriticRecurrent

REF = "/root/reference/source/robot_lab"
shims.install()
LSTM = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]


def _rule(name, **kw):
    r = dh.reference(name, **kw)["f64"]
    return dict(groups=[g["grads"] for g in r["groups"]], params=r["params"], final_state=r["final_state"], behavior=r["result"]["behavior"])


def _params(name):
    return {k: p.detach().numpy() for k, p in dh.trained_named(dh.case(name)[0])}  # (the policy does not depend on the batch's seed)


# ---- the rule against independent definitions ------------------------------------------------------------------------------------------------
def test_the_shapes_cover_the_group_logic():
    g = {n: dh.update_groups(s) for n, s in RULE_SHAPES.items()}
    assert g["wrap+left-over"] == ([(0, 1, 2), (3, 4, 0), (1, 2, 3)], (4,))                       # one group wraps, one step is left over
    assert g["two-boundaries"] == ([(0, 1, 0, 1, 0)], (1,))                                       # one group spans two epoch boundaries
    assert len(g["gl-1"][0]) == 10 and g["gl-1"][1] == ()
    assert g["one-group"] == ([tuple(range(5)) * 2], ())                                          # gradient length = T x epochs
    d = dh.done_pattern(5, 6)
    assert d[0].any() and (d[2] & d[3]).any() and d[3, 3:].all() and (~d[:4].any(0)).any() and d[4].any()


@pytest.mark.parametrize("max_grad_norm", [None, 0.05])
@pytest.mark.parametrize("name", list(RULE_SHAPES))
def test_rule_equals_the_numpy_restatement(name, max_grad_norm):
    """forward, the cell's backward formulas and the cuts written out by hand, clip and Adam: every group's gradient, the final state, the
    parameters and the statistic"""
    ref = _rule(name, max_grad_norm=max_grad_norm)
    got = dh.np_update(_params(name), dh.case(name, max_grad_norm=max_grad_norm)[1], RULE_SHAPES[name], max_grad_norm=max_grad_norm)
    assert len(got["groups"]) == len(ref["groups"]) == len(dh.update_groups(RULE_SHAPES[name])[0])
    assert dh.worst(got, ref) <= 1e-10
    assert abs(got["behavior"] - ref["behavior"]) <= 1e-10 * abs(ref["behavior"])


def test_rule_equals_the_numpy_restatement_under_huber():
    name = "wrap+left-over"
    ref = _rule(name, loss_type="huber")
    got = dh.np_update(_params(name), dh.case(name, "huber")[1], RULE_SHAPES[name], loss_type="huber")
    assert dh.worst(got, ref) <= 1e-10 and abs(got["behavior"] - ref["behavior"]) <= 1e-10 * abs(ref["behavior"])


@pytest.mark.parametrize("name", list(RULE_SHAPES))
def test_rule_equals_the_walk_through_nn_lstm(name):
    """split at the dones and at an epoch's first step, every piece one call of nn.LSTM, the carried state detached by hand"""
    pol, f = dh.case(name)
    ref = _rule(name)
    got = dh.walk_update(pol, dh.as_batch(f, torch.float64), RULE_SHAPES[name])
    assert len(got["groups"]) == len(ref["groups"])
    assert dh.worst(got, ref) <= 1e-10
    assert abs(got["behavior"] - ref["behavior"]) <= 1e-10 * abs(ref["behavior"])


def test_one_group_by_autograd_is_the_rule_s_group():
    """`torch_group` (what hands the GPU tier its fp32 yardstick per group) reproduces every group of the fp64 update from the recorded parameters and
    carried state"""
    name = "wrap+left-over"
    pol, f = dh.case(name)
    p64, b64 = copy.deepcopy(pol).double(), dh.as_batch(f, torch.float64)
    for g in dh.reference(name)["f64"]["groups"]:
        with torch.no_grad():
            for k, p in dh.trained_named(p64):
                p.copy_(g["params"][k])
        grads, means, out = dh.torch_group(p64, b64, g["steps"], g["state_in"])
        for k in grads:
            np.testing.assert_allclose(grads[k], g["grads"][k], rtol=0, atol=1e-12 * np.abs(g["grads"][k]).max())
        np.testing.assert_allclose(means, g["means"], rtol=0, atol=1e-13)
        assert torch.equal(out[0], g["state_out"][0])


def test_bias_gradients_are_equal_and_have_their_own_moments():
    name = "wrap+left-over"
    r = dh.reference(name)["f64"]
    for g in r["groups"]:
        assert np.array_equal(g["grads"]["memory_s.rnn.bias_ih_l0"], g["grads"]["memory_s.rnn.bias_hh_l0"])
    assert r["exp_avg"]["memory_s.rnn.bias_ih_l0"] is not r["exp_avg"]["memory_s.rnn.bias_hh_l0"]
    alg = dh.torch_alg(dh.case(name)[0], torch.float64, name)
    assert len(alg.optimizer.param_groups[0]["params"]) == 4 + 2 * 3
    assert [id(p) for p in alg.optimizer.param_groups[0]["params"]] == [id(p) for p in alg.policy.trained_parameters()]


def test_the_last_dones_are_never_read_and_the_teacher_is_not_evaluated():
    name = "wrap+left-over"
    pol, f = dh.case(name)
    outs = []
    for flip in (False, True):
        g = {k: np.array(v) for k, v in f.items()}
        if flip:
            g["dones"][-1] = ~g["dones"][-1]
        alg = dh.torch_alg(pol, torch.float64, name)
        for p in alg.policy.teacher.parameters():
            p.data.fill_(float("nan"))
        res = alg.update(dh.as_batch(g, torch.float64))
        outs.append((res["behavior"], [p.detach().clone() for p in alg.policy.trained_parameters()], alg.final_state))
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert torch.equal(outs[0][2][0], outs[1][2][0]) and np.isfinite(outs[0][0])


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------------
def _multiples(name, got):
    """the largest e / d over the tensors the GPU tier bounds (every group's gradient tensors, the parameters, the final state): e the distance of
    `got` from the fp64 rule, d the fp32 rule's"""
    r = dh.reference(name)
    worst = 0.0
    pairs = [(ga[k], g64["grads"][k], g32["grads"][k]) for ga, g64, g32 in zip(got["groups"], r["f64"]["groups"], r["f32"]["groups"]) for k in g64["grads"]]
    pairs += [(got["params"][k], r["f64"]["params"][k], r["f32"]["params"][k]) for k in r["f64"]["params"]]
    pairs += [(got["final_state"][k], r["f64"]["final_state"][k], r["f32"]["final_state"][k]) for k in ("h", "c")]
    for a, r64, r32 in pairs:
        scale = np.abs(r64).max()
        d = np.abs(r32 - r64).max() / scale
        assert d > 0
        worst = max(worst, np.abs(a - r64).max() / scale / d)
    return worst


@pytest.mark.parametrize("defect", DEFECTS)
def test_a_wrong_rule_misses_by_orders_of_magnitude(defect):
    name = "wrap+left-over"
    ref = _rule(name)
    got = dh.np_update(_params(name), dh.case(name)[1], RULE_SHAPES[name], defect=defect)
    w, m = dh.worst(got, ref), _multiples(name, got)
    print(f"{defect:<48}{w:12.1e}{m:12.1e} d")
    assert w >= 1e-10 * 1e6, (defect, w)  # six orders above the agreement asked of a right rule
    assert m >= 8 * 100, (defect, m)      # two orders above the bound used on the GPU
    assert _multiples(name, dh.np_update(_params(name), dh.case(name)[1], RULE_SHAPES[name])) <= 8


@pytest.mark.parametrize("name,defects", [("two-boundaries", (0, 2, 3, 4, 5, 6, 7)), ("gl-1", (1, 3, 4, 5, 7)), ("one-group", (0, 2, 3, 4, 5, 7))])
def test_the_other_shapes_bite_where_the_defect_can_show(name, defects):
    """(a single group has no group boundary behind it, gradient length 1 has no link inside a group, a case without left-over steps has none to
    back-propagate)"""
    ref = _rule(name)
    for i, defect in enumerate(DEFECTS):
        w = dh.worst(dh.np_update(_params(name), dh.case(name)[1], RULE_SHAPES[name], defect=defect), ref)
        assert (w >= 1e-4) if i in defects else (w <= 1e-10), (name, defect, w)


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def _policy(**kw):
    return StudentTeacherRecurrent(9, 11, 3, **{**dict(student_hidden=(8, 6), teacher_hidden=(7,), init_noise_std=0.1, rnn_hidden_dim=5), **kw})


def test_state_dict_keys_and_trained_parameter_order():
    pol = _policy()
    keys = list(pol.state_dict())
    want = ([f"memory_s.rnn.{k}" for k in LSTM] + [f"student.{2 * l}.{k}" for l in range(3) for k in ("weight", "bias")] + [f"memory_t.rnn.{k}" for k in LSTM] +
            [f"teacher.{2 * l}.{k}" for l in range(2) for k in ("weight", "bias")] + ["std"])
    assert sorted(keys) == sorted(want)
    names = {id(p): k for k, p in pol.named_parameters()}
    assert [names[id(p)] for p in pol.trained_parameters()] == want[:10]
    assert not any(p.requires_grad for k, p in pol.named_parameters() if k.startswith(("teacher.", "memory_t.")))
    ff = _policy(teacher_recurrent=False)
    assert not any(k.startswith("memory_t.") for k in ff.state_dict()) and ff.teacher[0].in_features == 11 and pol.teacher[0].in_features == 5
    norm = _policy(teacher_obs_normalization=True)
    assert any(k.startswith("teacher_obs_normalizer.") for k in norm.state_dict())
    with pytest.raises(NotImplementedError, match="gru"):
        _policy(rnn_type="gru")
    with pytest.raises(NotImplementedError, match="rnn_num_layers"):
        _policy(rnn_num_layers=2)


def test_load_state_dict_three_cases_and_the_mismatches():
    torch.manual_seed(0)
    rec = ActorCriticRecurrent(11, 13, 3, actor_hidden=(7,), critic_hidden=(4,), rnn_hidden_dim=5).state_dict()
    from robot_lab_amd.ppo import ActorCritic

    ff = ActorCritic(11, 13, 3, actor_hidden=(7,), critic_hidden=(4,)).state_dict()
    # a recurrent PPO checkpoint becomes a recurrent teacher
    pol = _policy()
    before = copy.deepcopy(pol.state_dict())
    assert pol.load_state_dict(rec) is False and pol.loaded_teacher
    for k in LSTM:
        assert torch.equal(pol.memory_t.rnn.state_dict()[k], rec[f"memory_a.rnn.{k}"])
    assert torch.equal(pol.teacher[0].weight, rec["actor.0.weight"]) and torch.equal(pol.teacher[2].bias, rec["actor.2.bias"])
    assert all(torch.equal(pol.state_dict()[k], before[k]) for k in before if k.startswith(("student.", "memory_s.", "std")))
    assert not pol.teacher.training
    # a feed-forward PPO checkpoint becomes a feed-forward teacher
    pol_ff = _policy(teacher_recurrent=False)
    assert pol_ff.load_state_dict(ff) is False and torch.equal(pol_ff.teacher[0].weight, ff["actor.0.weight"])
    # the kind must match teacher_recurrent; the message names the keyword
    with pytest.raises(RuntimeError, match="teacher_recurrent=True"):
        _policy(teacher_recurrent=False).load_state_dict(rec)
    with pytest.raises(RuntimeError, match="teacher_recurrent=False"):
        _policy().load_state_dict(ff)
    # strict on shapes
    with pytest.raises(RuntimeError):
        _policy(rnn_hidden_dim=6).load_state_dict(rec)
    with pytest.raises(RuntimeError, match="teacher_obs_normalization=False"):
        _policy(teacher_obs_normalization=True).load_state_dict(rec)
    # a distillation checkpoint resumes
    other = _policy()
    assert other.load_state_dict(pol.state_dict()) is True and other.loaded_teacher
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), pol.state_dict().values()))
    with pytest.raises(RuntimeError, match="teacher_recurrent=True"):
        _policy(teacher_recurrent=False).load_state_dict(pol.state_dict())
    with pytest.raises(RuntimeError, match="teacher_recurrent=False"):
        _policy().load_state_dict(pol_ff.state_dict())
    from robot_lab_amd.distill import StudentTeacher

    with pytest.raises(RuntimeError, match="feed-forward student"):
        _policy().load_state_dict(StudentTeacher(9, 11, 3, (8, 6), (7,)).state_dict())
    with pytest.raises(ValueError, match="neither actor"):
        _policy().load_state_dict({"foo": torch.zeros(1)})


def test_the_rule_refuses_what_it_is_not():
    with pytest.raises(TypeError, match="StudentTeacherRecurrent"):
        RecurrentDistillation(object())
    with pytest.raises(ValueError, match=">= 1"):
        RecurrentDistillation(_policy(), gradient_length=0)
    with pytest.raises(ValueError, match="loss_type"):
        RecurrentDistillation(_policy(), loss_type="l1")


# ---- the reference's cfg ---------------------------------------------------------------------------------------------------------------------
M = dict(class_name="MLPModel", hidden_dims=[128, 128, 128], activation="elu", obs_normalization=False, distribution_cfg=dict(init_std=0.1))
R = dict(M, class_name="RNNModel", rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)
CFG = dict(class_name="DistillationRunner", num_steps_per_env=120, seed=42, obs_groups={"student": ["policy"], "teacher": ["policy"]}, student=R, teacher=R,
           algorithm=dict(class_name="Distillation", num_learning_epochs=2, learning_rate=1e-3, gradient_length=15, optimizer="adam", loss_type="mse"))


def _check_reference_numbers(kw):
    assert kw["rnn_type"] == "lstm" and kw["rnn_hidden_dim"] == 256 and kw["rnn_num_layers"] == 1 and kw["teacher_recurrent"] is True
    assert kw["student_hidden"] == (128, 128, 128) and kw["teacher_hidden"] == (128, 128, 128)
    assert kw["num_steps_per_env"] == 120 and kw["gradient_length"] == 15 and kw["num_learning_epochs"] == 2 and kw["learning_rate"] == 1e-3
    assert kw["init_noise_std"] == 0.1 and kw["student_group"] == kw["teacher_group"] == "policy" and kw["loss_type"] == "mse"


def test_the_cfg_in_the_reference_s_spelling_reads():
    from rsl_rl.runners import is_recurrent_distillation_cfg, read_distillation_cfg, read_recurrent_distillation_cfg

    assert is_recurrent_distillation_cfg(CFG) and not is_recurrent_distillation_cfg(dict(CFG, student=M, teacher=M))
    assert is_recurrent_distillation_cfg(dict(CFG, teacher=M)) and is_recurrent_distillation_cfg(dict(CFG, student=M))
    _check_reference_numbers(read_recurrent_distillation_cfg(CFG))
    assert read_recurrent_distillation_cfg(dict(CFG, teacher=M))["teacher_recurrent"] is False
    with pytest.raises(NotImplementedError, match="recurrent"):  # the feed-forward reader stays what it was
        read_distillation_cfg(CFG)


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's cfg file")
def test_reference_recurrent_distillation_cfg_imports_unchanged_and_reads():
    shims.install(shims.REFERENCE_SOURCE)
    import importlib

    from rsl_rl.runners import is_recurrent_distillation_cfg, read_distillation_cfg, read_recurrent_distillation_cfg

    mod = importlib.import_module("robot_lab.tasks.manager_based.locomotion.velocity.config.quadruped.anymal_d.agents.rsl_rl_distillation_cfg")
    d = mod.AnymalDFlatDistillationRunnerRecurrentCfg().to_dict()
    assert d["class_name"] == "DistillationRunner" and is_recurrent_distillation_cfg(d)
    _check_reference_numbers(read_recurrent_distillation_cfg(d))
    with pytest.raises(NotImplementedError, match="recurrent"):
        read_distillation_cfg(d)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,exc,reason", [
    (dict(student=M), NotImplementedError, "feed-forward student with a recurrent teacher"),
    (dict(student=dict(R, rnn_type="gru"), teacher=dict(R, rnn_type="gru")), NotImplementedError, "gru"),
    (dict(student=dict(R, rnn_num_layers=2), teacher=dict(R, rnn_num_layers=2)), NotImplementedError, "rnn_num_layers"),
    (dict(student=dict(R, rnn_hidden_dim=1024), teacher=dict(R, rnn_hidden_dim=1024)), ValueError, "1..512"),
    (dict(teacher=dict(R, rnn_hidden_dim=128)), NotImplementedError, "rnn settings differ"),
    (dict(student=dict(R, class_name="MLPModel")), NotImplementedError, "class_name=\"RNNModel\""),
    (dict(student=dict(R, activation="relu")), NotImplementedError, "ELU"),
    (dict(teacher=dict(R, activation="tanh")), NotImplementedError, "ELU"),
    (dict(student=dict(R, obs_normalization=True)), NotImplementedError, "student obs_normalization"),
    (dict(student={k: v for k, v in R.items() if k != "hidden_dims"}), ValueError, "hidden_dims"),
    (dict(student=None), ValueError, "no `student`"),
    (dict(policy=dict(class_name="StudentTeacherRecurrent")), NotImplementedError, "rsl_rl 3.0.1's spelling"),
    (dict(algorithm=dict(class_name="PPO")), NotImplementedError, "Distillation"),
    (dict(algorithm=dict(optimizer="sgd")), NotImplementedError, "adam"),
    (dict(obs_groups={"student": ["policy", "critic"]}), NotImplementedError, "exactly one observation group"),
    (dict(obs_groups={"teacher": ["privileged"]}), ValueError, "no observation group"),
])
def test_the_reader_refuses_with_a_reason(change, exc, reason):
    from rsl_rl.runners import read_recurrent_distillation_cfg

    with pytest.raises(exc, match=reason):
        read_recurrent_distillation_cfg({**CFG, **change})


class NoEnv:
    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the refusal")


def test_trainer_refusals_come_before_the_env_is_touched():
    from robot_lab_amd.distill import DistillTrainer

    for kw, exc, reason in ((dict(rnn_type="gru"), NotImplementedError, "gru"), (dict(rnn_type="lstm", rnn_num_layers=2), NotImplementedError, "rnn_num_layers"),
                            (dict(teacher_recurrent=True), NotImplementedError, "feed-forward student with a recurrent teacher"),
                            (dict(rnn_type="lstm", rnn_hidden_dim=513), ValueError, "outside 1..512"), (dict(rnn_type="rnn"), ValueError, "must be \"lstm\""),
                            (dict(rnn_type="lstm", learner="cuda"), ValueError, "learner must be")):
        with pytest.raises(exc, match=reason):
            DistillTrainer(NoEnv(), **kw)


def test_the_runner_routes_on_the_cfg_and_keeps_its_first_refusal(monkeypatch):
    from rsl_rl.runners import DistillationRunner

    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(NotImplementedError, match="2 ranks"):  # still the first check, before the cfg is read or the env touched
        DistillationRunner(NoEnv(), dict(CFG, student=dict(R, rnn_type="gru")), device="cpu")
