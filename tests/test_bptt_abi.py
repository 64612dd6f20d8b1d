"""CPU tier of the recurrent learner's C-ABI (include/rl_bptt.h, robot_lab_amd/recurrent_hip.py): header, library and binding agree, the struct
mirrors match the header, `rl_bptt_create` refuses what it cannot do before a device is touched, the flat layout is the order of
`ActorCriticRecurrent.parameters()`, and the public switch (`recurrent_learner=`, `RL_RECURRENT_LEARNER`) refuses before the env is touched.
The numerics are tests/test_bptt_rule.py (CPU) and tests/test_gpu_bptt.py."""
import ctypes as C
import os
import re

import pytest

from robot_lab_amd import recurrent_hip as rh
from robot_lab_amd.capi import PPO_LIB, Hyper
from robot_lab_amd.recurrent import ActorCriticRecurrent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(name):
    return re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)


def test_header_library_and_binding_agree():
    declared = sorted(set(re.findall(r"\b(rl_bptt_[a-z_]+)\s*\(", _code("rl_bptt.h"))))
    assert len(declared) == 15
    raw = C.CDLL(PPO_LIB)
    for name in declared:
        assert hasattr(raw, name), f"librl_ppo_hip.so does not export {name}"
    assert declared == sorted(rh.BPTT_EXPORTS)
    bound = rh.load_bptt_library()
    for name in declared:
        assert getattr(bound, name).argtypes is not None or name == "rl_bptt_last_error", name
    src = _header("rl_bptt.h")
    assert int(re.search(r"#define RL_BPTT_MAX_LAYERS (\d+)", src).group(1)) == rh.MAX_LAYERS == 8
    assert int(re.search(r"#define RL_BPTT_MAX_WIDTH (\d+)", src).group(1)) == rh.MAX_WIDTH == 512
    assert int(re.search(r"#define RL_BPTT_STATS (\d+)", src).group(1)) == 8
    # prototypes: as many ctypes arguments as the header declares parameters
    for name in declared:
        params = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", _code("rl_bptt.h"), flags=re.S).group(1)
        n = 0 if params.strip() == "void" else params.count(",") + 1
        if name != "rl_bptt_last_error":
            assert len(getattr(bound, name).argtypes) == n, name


def _struct_fields(header, struct):
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", _code(header), flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for name in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl[re.match(r"(const\s+)?\w+", decl).end():]):
            out.append((name, ctype, "*" in decl))
    return out


def test_struct_mirrors_match_the_header():
    batch = _struct_fields("rl_bptt.h", "rl_bptt_batch")
    assert [n for n, _, _ in batch] == [n for n, _ in rh.BpttBatch._fields_]
    assert all(ptr for _, _, ptr in batch) and all(t is C.c_void_p for _, t in rh.BpttBatch._fields_)
    assert dict((n, t) for n, t, _ in batch)["dones"] == "uint8_t"
    assert C.sizeof(rh.BpttBatch) == 14 * C.sizeof(C.c_void_p)
    ctypes_of = {"double": C.c_double, "float": C.c_float, "int32_t": C.c_int32}
    hyper = _struct_fields("rl_ppo.h", "rl_ppo_hyper")
    assert [(n, ctypes_of[t]) for n, t, _ in hyper] == list(Hyper._fields_)
    assert '#include "rl_ppo.h"' in _header("rl_bptt.h")  # the hyper-parameters are the PPO learner's struct, not a copy


def _hyper(**kw):
    base = dict(learning_rate=1e-3, desired_kl=0.01, value_loss_coef=1.0, clip_param=0.2, entropy_coef=0.01, max_grad_norm=1.0, use_clipped_value_loss=1,
                num_learning_epochs=2, num_mini_batches=2, schedule=1, std_type=0)
    return Hyper(**{**base, **kw})


def _create(obs=45, cobs=50, hidden=20, actor=(20, 32, 12), critic=(20, 32, 1), activation=0, T=5, N=8, **hp):
    lib = rh.load_bptt_library()
    out = C.c_void_p(0xdead)
    n = len(actor) - 1
    rc = lib.rl_bptt_create(obs, cobs, hidden, (C.c_int32 * len(actor))(*actor), (C.c_int32 * len(critic))(*critic), n, activation, C.byref(_hyper(**hp)), T, N, 0,
                            C.byref(out))
    return rc, out.value, lib.rl_bptt_last_error().decode()


@pytest.mark.parametrize("kw,reason", [
    (dict(obs=0), "width 0"), (dict(obs=513), "width 513"), (dict(cobs=513), "width 513"), (dict(hidden=513, actor=(513, 8, 2), critic=(513, 8, 1)), "width 513"),
    (dict(hidden=0, actor=(0, 8, 2), critic=(0, 8, 1)), "width 0"), (dict(actor=(20, 513, 12)), "layer width 513"), (dict(critic=(20, 0, 1)), "layer width"),
    (dict(actor=(20,) + (8,) * 9, critic=(20,) + (8,) * 8 + (1,)), "layer count 9"), (dict(activation=1), "ELU"), (dict(activation=2), "ELU"),
    (dict(std_type=1), "scalar"), (dict(schedule=1, desired_kl=0.0), "desired_kl"), (dict(schedule=1, desired_kl=-1.0), "desired_kl"),
    (dict(N=1, num_mini_batches=2), "num_envs < num_mini_batches"), (dict(T=0), "T 0"), (dict(actor=(16, 32, 12)), "hidden size"), (dict(critic=(20, 32, 2)), "output width"),
])
def test_create_refuses_with_a_reason_and_a_null_handle(kw, reason):
    rc, handle, err = _create(**kw)
    assert rc != 0 and not handle and reason in err, (rc, handle, err)


def test_create_checks_its_arguments_before_the_device():
    """a valid request gets as far as the device: without one that is the refusal; with one a handle"""
    rc, handle, err = _create()
    if rc != 0:
        assert not handle and "hipSetDevice" in err, err
    else:
        assert handle
        rh.load_bptt_library().rl_bptt_destroy(C.c_void_p(handle))


def test_flat_order_is_the_order_of_parameters():
    pol = ActorCriticRecurrent(45, 50, 12, actor_hidden=(32, 16), critic_hidden=(24, 8), rnn_hidden_dim=20)
    names = [k for k, _ in pol.named_parameters()]
    lstm = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    assert names == (["std"] + [f"memory_a.rnn.{k}" for k in lstm] + [f"memory_c.rnn.{k}" for k in lstm] +
                     [f"actor.{2 * l}.{k}" for l in range(3) for k in ("weight", "bias")] + [f"critic.{2 * l}.{k}" for l in range(3) for k in ("weight", "bias")])
    shapes = rh.recurrent_parameter_shapes(45, 50, 20, [20, 32, 16, 12], [20, 24, 8, 1])
    assert shapes == [tuple(p.shape) for p in pol.parameters()]
    # ... and the header says so, in this order
    doc = _header("rl_bptt.h")
    order = [doc.index(w) for w in ("std[act]; memory_a weight_ih", "weight_hh [4H][H]", "bias_ih [4H]", "bias_hh [4H]; memory_c", "per actor layer", "the critic's layers alike")]
    assert order == sorted(order)


def test_other_headers_do_not_know_the_recurrent_learner():
    for h in ("rl_ppo.h", "rl_distill.h", "rl_lstm.h"):
        assert "rl_bptt_" not in _header(h), h


class NoEnv:
    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the refusal")


def test_recurrent_learner_refusals_come_before_the_env_is_touched():
    from robot_lab_amd.ppo import Trainer

    with pytest.raises(ValueError, match="recurrent_learner must be"):
        Trainer(NoEnv(), rnn_type="lstm", recurrent_learner="cuda")
    with pytest.raises(ValueError, match="recurrent_learner must be"):
        Trainer(NoEnv(), recurrent_learner="cuda")
    with pytest.raises(NotImplementedError, match="recurrent policy only"):
        Trainer(NoEnv(), recurrent_learner="hip")
    # the pinned refusal of learner="hip" stays, and points to the switch
    with pytest.raises(NotImplementedError, match="back-propagation through time.*recurrent_learner=\"hip\""):
        Trainer(NoEnv(), rnn_type="lstm", learner="hip")
    with pytest.raises(NotImplementedError, match="back-propagation through time"):
        Trainer(NoEnv(), rnn_type="lstm", learner="hip", recurrent_learner="hip")
    group = type("G", (), {"world_size": 2})()
    for kw, reason in ((dict(rnn_type="gru"), "gru"), (dict(rnn_num_layers=2), "rnn_num_layers"), (dict(symmetry="lr"), "symmetry"),
                       (dict(actor_obs_normalization=True), "normalisation"), (dict(group=group), "2 ranks")):
        with pytest.raises(NotImplementedError, match=reason):
            Trainer(NoEnv(), **{"rnn_type": "lstm", "recurrent_learner": "hip", **kw})


def test_runner_switch_is_read_from_the_environment(monkeypatch):
    import recurrent_helpers
    from robot_lab_amd.shims.rsl_rl.runners import OnPolicyRunner, recurrent_learner_from_env

    assert recurrent_learner_from_env({}) == "torch" and recurrent_learner_from_env({"RL_RECURRENT_LEARNER": "hip"}) == "hip"
    with pytest.raises(ValueError, match="RL_RECURRENT_LEARNER"):
        recurrent_learner_from_env({"RL_RECURRENT_LEARNER": "HIP"})
    monkeypatch.setenv("RL_RECURRENT_LEARNER", "rocm")
    with pytest.raises(ValueError, match="RL_RECURRENT_LEARNER='rocm'"):
        OnPolicyRunner(object(), recurrent_helpers.RSL_RL_SPELLING, device="cpu")
    monkeypatch.setenv("RL_RECURRENT_LEARNER", "hip")
    monkeypatch.setenv("RL_LEARNER", "hip")
    with pytest.raises(NotImplementedError, match="RL_LEARNER=hip with a recurrent cfg.*RL_RECURRENT_LEARNER=hip"):
        OnPolicyRunner(object(), recurrent_helpers.RSL_RL_SPELLING, device="cpu")


def test_learner_refusals_need_no_device():
    pol = ActorCriticRecurrent(5, 6, 2, actor_hidden=(8,), critic_hidden=(8,), rnn_hidden_dim=4)
    with pytest.raises(NotImplementedError, match="symmetry"):
        rh.HipRecurrentPPO(pol, symmetry=object())
    with pytest.raises(NotImplementedError, match="group"):
        rh.HipRecurrentPPO(pol, group=type("G", (), {"world_size": 4})())
    with pytest.raises(TypeError, match="ActorCriticRecurrent"):
        rh.HipRecurrentPPO(object())
    with pytest.raises(ValueError, match="one CUDA device"):
        rh.HipRecurrentPPO(pol)
    with pytest.raises(ValueError, match="desired_kl"):
        rh.HipRecurrentPPO(pol, desired_kl=0.0)
