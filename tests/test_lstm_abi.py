"""CPU tier of the LSTM cell's C-ABI (include/rl_lstm.h, robot_lab_amd/lstm.py) and of the recurrent cfgs: header, library and binding
agree, both cfg spellings translate to the same `Trainer` keywords, and everything that is refused without a device is refused with its
reason.  The numerics are tests/test_gpu_lstm_exact.py, the device-side refusals tests/test_gpu_recurrent.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import recurrent_helpers as rh
from robot_lab_amd import lstm
from robot_lab_amd.recurrent import ActorCriticRecurrent, RecurrentPPO, read_recurrent_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree():
    declared = _declared("rl_lstm.h", "rl_lstm_")
    assert len(declared) == 8
    lib = C.CDLL(lstm.LSTM_LIB)
    for name in declared:
        assert hasattr(lib, name), f"librl_lstm_hip.so does not export {name}"
    assert declared == sorted(lstm.LSTM_EXPORTS)
    bound = lstm.load_lstm_library()
    for name in declared:
        assert getattr(bound, name).argtypes is not None or name == "rl_lstm_last_error", name
    src = open(os.path.join(ROOT, "include", "rl_lstm.h")).read()
    assert int(re.search(r"#define RL_LSTM_MAX_WIDTH (\d+)", src).group(1)) == lstm.MAX_WIDTH == 512


def test_create_refuses_before_touching_a_device():
    lib = lstm.load_lstm_library()
    w = np.zeros(4, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))
    for d, h in ((0, 4), (513, 4), (4, 0), (4, 513)):
        out = C.c_void_p()
        assert lib.rl_lstm_create(d, h, w, w, w, w, 0, C.byref(out)) != 0 and not out.value
        assert "out of range" in lib.rl_lstm_last_error().decode()
    out = C.c_void_p()
    assert lib.rl_lstm_create(4, 4, None, w, w, w, 0, C.byref(out)) != 0 and "null" in lib.rl_lstm_last_error().decode()


def test_binding_checks_shapes_before_the_library():
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    assert lstm.check_lstm_shapes(z(80, 45), z(80, 20), z(80), z(80)) == (45, 20)
    with pytest.raises(ValueError, match="weight_hh"):
        lstm.check_lstm_shapes(z(80, 45), z(80, 21), z(80), z(80))
    with pytest.raises(ValueError, match="weight_ih"):
        lstm.check_lstm_shapes(z(84, 45), z(80, 20), z(80), z(80))
    with pytest.raises(ValueError, match="biases"):
        lstm.check_lstm_shapes(z(80, 45), z(80, 20), z(80), z(79))
    with pytest.raises(ValueError, match="out of range"):
        lstm.check_lstm_shapes(z(80, 513), z(80, 20), z(80), z(80))


# ---- the cfg translation -----------------------------------------------------------------------------------------------------------------
RSL_RL_SPELLING, REFERENCE_SPELLING = rh.RSL_RL_SPELLING, rh.REFERENCE_SPELLING


def test_both_spellings_give_the_same_keywords():
    want = dict(actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 64), init_noise_std=0.8, rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1,
                critic_group="critic")
    assert read_recurrent_cfg(RSL_RL_SPELLING) == want
    assert read_recurrent_cfg(REFERENCE_SPELLING) == want
    shared = dict(REFERENCE_SPELLING, obs_groups={"actor": ["policy"], "critic": ["policy"]})
    assert read_recurrent_cfg(shared) == dict(want, critic_group="policy")


def test_a_feed_forward_cfg_is_not_recurrent():
    assert read_recurrent_cfg(dict(policy=dict(class_name="ActorCritic", actor_hidden_dims=[512, 256, 128]), algorithm={})) is None
    assert read_recurrent_cfg({}) is None


def _with(base, **changes):
    import copy

    cfg = copy.deepcopy(base)
    for path, v in changes.items():
        d = cfg
        *head, last = path.split("__")
        for k in head:
            d = d[k]
        d[last] = v
    return cfg


@pytest.mark.parametrize("cfg,exc,reason", [
    (_with(RSL_RL_SPELLING, policy__rnn_type="gru"), NotImplementedError, "gru"),
    (_with(RSL_RL_SPELLING, policy__rnn_num_layers=2), NotImplementedError, "rnn_num_layers"),
    (_with(RSL_RL_SPELLING, policy__rnn_hidden_dim=1024), ValueError, "rnn_hidden_dim"),
    (_with(RSL_RL_SPELLING, policy__actor_obs_normalization=True), NotImplementedError, "normalisation"),
    (_with(RSL_RL_SPELLING, policy__activation="tanh"), NotImplementedError, "ELU"),
    (_with(RSL_RL_SPELLING, obs_groups={"policy": ["policy", "critic"]}), NotImplementedError, "obs_groups"),
    (_with(REFERENCE_SPELLING, critic__rnn_hidden_dim=128), NotImplementedError, "differ"),
    (_with(REFERENCE_SPELLING, critic__class_name="MLPModel", critic__rnn_type=None), NotImplementedError, "feed-forward critic"),
    (_with(REFERENCE_SPELLING, actor__obs_normalization=True), NotImplementedError, "obs_normalization"),
    (_with(REFERENCE_SPELLING, actor__rnn_type="gru", critic__rnn_type="gru"), NotImplementedError, "gru"),
])
def test_cfg_refusals_carry_their_reason(cfg, exc, reason):
    with pytest.raises(exc, match=reason):
        read_recurrent_cfg(cfg)


# ---- refusals that need no device --------------------------------------------------------------------------------------------------------
def test_trainer_refusals_come_before_the_env_is_touched():
    from robot_lab_amd.ppo import Trainer

    class NoEnv:
        def __getattr__(self, name):
            raise AssertionError(f"the env was touched ({name}) before the refusal")

    group = type("G", (), {"world_size": 2})()
    for kw, exc, reason in ((dict(learner="hip"), NotImplementedError, "back-propagation through time"), (dict(rnn_type="gru"), NotImplementedError, "gru"),
                            (dict(rnn_num_layers=2), NotImplementedError, "rnn_num_layers"), (dict(symmetry="lr"), NotImplementedError, "symmetry"),
                            (dict(actor_obs_normalization=True), NotImplementedError, "normalisation"), (dict(critic_obs_normalization=True), NotImplementedError, "normalisation"),
                            (dict(group=group), NotImplementedError, "2 ranks"), (dict(critic_group="teacher"), ValueError, "critic_group")):
        with pytest.raises(exc, match=reason):
            Trainer(NoEnv(), **{"rnn_type": "lstm", **kw})
    with pytest.raises(NotImplementedError, match="recurrent policy only"):
        Trainer(NoEnv(), critic_group="policy")


def test_collector_refusals_need_no_device():
    from robot_lab_amd.collect import Collector

    for kw, reason in ((dict(overlap=True), "overlap=True"), (dict(fused_act=True), "fused_act"), (dict(normalizers=(object(), None)), "normalizers")):
        with pytest.raises(NotImplementedError, match=reason):
            Collector(None, None, None, None, None, recurrent=object(), **kw)


def test_learner_refusals():
    pol = ActorCriticRecurrent(5, 6, 2, actor_hidden=(8,), critic_hidden=(8,), rnn_hidden_dim=4)
    with pytest.raises(NotImplementedError, match="symmetry"):
        RecurrentPPO(pol, symmetry=object())
    with pytest.raises(NotImplementedError, match="group"):
        RecurrentPPO(pol, group=type("G", (), {"world_size": 4})())
    with pytest.raises(ValueError, match="do not fill"):
        RecurrentPPO(pol, num_mini_batches=4).blocks(3)
    with pytest.raises(NotImplementedError, match="gru"):
        ActorCriticRecurrent(5, 6, 2, rnn_type="gru")
    with pytest.raises(NotImplementedError, match="rnn_num_layers"):
        ActorCriticRecurrent(5, 6, 2, rnn_num_layers=3)


def test_runner_refuses_the_hip_learner_for_a_recurrent_cfg(monkeypatch):
    from robot_lab_amd.shims.rsl_rl.runners import OnPolicyRunner

    monkeypatch.setenv("RL_LEARNER", "hip")
    for cfg in (RSL_RL_SPELLING, REFERENCE_SPELLING):
        with pytest.raises(NotImplementedError, match="RL_LEARNER=hip with a recurrent cfg"):
            OnPolicyRunner(object(), cfg, device="cpu")


def test_distillation_runner_still_refuses_recurrent_models():
    from robot_lab_amd.shims.rsl_rl.runners import read_distillation_cfg

    m = dict(hidden_dims=[64], activation="elu")
    with pytest.raises(NotImplementedError, match="recurrent"):
        read_distillation_cfg(dict(student=dict(m, class_name="RNNModel", rnn_type="lstm"), teacher=m, algorithm={}))


def test_exporters_refuse_a_recurrent_policy(tmp_path):
    from robot_lab_amd import shims

    shims.install()
    from isaaclab_rl.rsl_rl import export_policy_as_jit, export_policy_as_onnx

    pol = ActorCriticRecurrent(5, 6, 2, actor_hidden=(8,), critic_hidden=(8,), rnn_hidden_dim=4)
    with pytest.raises(NotImplementedError, match="recurrent policy"):
        export_policy_as_jit(pol, path=str(tmp_path))
    try:
        import onnx  # noqa: F401
    except ImportError:
        return  # (the ONNX exporter asks for the package first, as upstream does)
    with pytest.raises(NotImplementedError, match="recurrent policy"):
        export_policy_as_onnx(pol, path=str(tmp_path))
