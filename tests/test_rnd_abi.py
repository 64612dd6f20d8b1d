"""CPU tier of the two RND libraries (include/rl_rnd.h -> librl_rnd_hip.so, include/rl_rnd_learner.h -> librl_ppo_hip.so; robot_lab_amd/rnd_hip.py):
headers, libraries and binding agree on the `rl_rnd_*` names, and every create-time refusal carries its reason with no device present - both
`create` functions check their arguments before they touch one.  The numerics are tests/test_gpu_rnd.py."""
import ctypes as C
import os
import re

import pytest

from robot_lab_amd import rnd_hip
from robot_lab_amd.rnd import RandomNetworkDistillation
from robot_lab_amd.rnd_hip import RND_LEARNER_EXPORTS, RND_REWARD_EXPORTS, HipRND, RndHyper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declared(name):
    return sorted(set(re.findall(r"\b(rl_rnd_[a-z_]+)\s*\(", _header(name))))


def test_reward_header_library_and_binding_agree():
    declared = _declared("rl_rnd.h")
    assert len(declared) == 10 and all(n.startswith("rl_rnd_reward_") for n in declared)
    lib = C.CDLL(rnd_hip.RND_LIB)
    for name in declared:
        assert hasattr(lib, name), f"librl_rnd_hip.so does not export {name}"
    assert declared == sorted(RND_REWARD_EXPORTS)
    bound = rnd_hip.load_rnd_reward_library()
    for name in declared:
        assert getattr(bound, name).argtypes is not None or name == "rl_rnd_reward_last_error", name
    assert int(re.search(r"#define RL_RND_MAX_OUTPUTS (\d+)", _header("rl_rnd.h")).group(1)) == rnd_hip.MAX_OUTPUTS == 512


def test_learner_header_library_and_binding_agree():
    declared = _declared("rl_rnd_learner.h")
    assert len(declared) == 14 and not any(n.startswith("rl_rnd_reward_") for n in declared)
    lib = C.CDLL(rnd_hip.PPO_LIB)  # the learner library: next to the PPO learner
    for name in declared:
        assert hasattr(lib, name), f"librl_ppo_hip.so does not export {name}"
    assert declared == sorted(RND_LEARNER_EXPORTS)
    bound = rnd_hip.load_rnd_learner_library()
    for name in declared:
        assert getattr(bound, name).argtypes is not None or name == "rl_rnd_last_error", name
    assert not hasattr(C.CDLL(rnd_hip.RND_LIB), "rl_rnd_update")  # each name lives in one library


def test_hyper_struct_mirrors_the_header():
    body = re.search(r"typedef struct rl_rnd_hyper \{(.*?)\}", _header("rl_rnd_learner.h"), flags=re.S).group(1)
    names = [n.strip(" *\n") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in RndHyper._fields_]
    assert C.sizeof(RndHyper) == 16


def test_nothing_was_added_to_the_rollout_and_ppo_headers():
    for header in ("rl_rollout.h", "rl_ppo.h", "rl_distill.h"):
        assert "rl_rnd" not in open(os.path.join(ROOT, "include", header)).read(), header
    from robot_lab_amd.rollout import ROLLOUT_EXPORTS

    assert not any("rnd" in n for n in ROLLOUT_EXPORTS)


def test_reward_create_refuses_before_touching_a_device():
    lib = rnd_hip.load_rnd_reward_library()

    def create(num_envs=64, num_outputs=4, num_steps=24, gamma=0.99):
        out = C.c_void_p(0xdead)
        assert lib.rl_rnd_reward_create(num_envs, num_outputs, num_steps, gamma, 0, C.byref(out)) != 0 and not out.value  # a reason and a null handle
        return lib.rl_rnd_reward_last_error().decode()

    assert "num_envs" in create(num_envs=0)
    assert "num_outputs" in create(num_outputs=0)
    assert "num_outputs" in create(num_outputs=513)
    assert "num_steps" in create(num_steps=0)
    for g in (-0.1, 1.5, float("nan"), float("inf")):
        assert "gamma_r" in create(gamma=g)
    assert lib.rl_rnd_reward_create(64, 4, 24, 0.99, 0, None) != 0 and "null" in lib.rl_rnd_reward_last_error().decode()
    assert lib.rl_rnd_reward_sums(None, 1, None, None) != 0 and "null" in lib.rl_rnd_reward_last_error().decode()


def test_learner_create_refuses_before_touching_a_device():
    lib = rnd_hip.load_rnd_learner_library()

    def create(pdims, tdims=None, act=0, max_rows=64, **hyper):
        tdims = tdims or pdims
        kw = dict(learning_rate=1e-3, num_learning_epochs=2, num_mini_batches=2)
        kw.update(hyper)
        hp, out = RndHyper(**kw), C.c_void_p(0xdead)
        rc = lib.rl_rnd_create((C.c_int32 * len(pdims))(*pdims), len(pdims) - 1, (C.c_int32 * len(tdims))(*tdims), len(tdims) - 1, act, C.byref(hp), max_rows, 0,
                               C.byref(out))
        assert rc != 0 and not out.value
        return lib.rl_rnd_last_error().decode()

    assert "activation" in create([45, 64, 4], act=1)
    assert "activation" in create([45, 64, 4], act=2)
    assert "width" in create([45, 1024, 4]) and "predictor" in create([45, 1024, 4])
    assert "width" in create([45, 64, 4], [45, 0, 4]) and "target" in create([45, 64, 4], [45, 0, 4])
    assert "width" in create([513, 64, 4])
    assert "layer count" in create([45] * 10)
    assert "layer count" in create([45, 8, 45], [45] * 10)
    assert "differ" in create([45, 64, 4], [45, 64, 5])
    assert "differ" in create([45, 64, 4], [44, 64, 4])
    for lr in (0.0, -1e-3, float("inf"), float("nan")):
        assert "learning rate" in create([45, 64, 4], learning_rate=lr)
    assert "num_learning_epochs" in create([45, 64, 4], num_learning_epochs=0)
    assert "num_mini_batches" in create([45, 64, 4], num_mini_batches=0)
    assert "max_rows_per_minibatch" in create([45, 64, 4], max_rows=0)


def test_python_class_refuses_with_a_reason():
    from torch import nn

    from robot_lab_amd.ppo import mlp

    m = RandomNetworkDistillation(10, num_outputs=2, predictor_hidden_dims=(16,), target_hidden_dims=(16,))
    with pytest.raises(ValueError, match="CUDA device"):  # no CPU path and no fall-back
        HipRND(m, max_rows_per_minibatch=8)
    with pytest.raises(ValueError, match="state_normalizer"):
        HipRND(RandomNetworkDistillation(10, predictor_hidden_dims=(16,), target_hidden_dims=(16,), state_normalization=True), max_rows_per_minibatch=8)
    m.predictor = mlp([10, 16, 2], activation=nn.Tanh)
    with pytest.raises(ValueError, match="unsupported activation"):
        HipRND(m, max_rows_per_minibatch=8)
    with pytest.raises(ValueError, match="width <= 512"):
        HipRND(RandomNetworkDistillation(10, predictor_hidden_dims=(1024,), target_hidden_dims=(16,)), max_rows_per_minibatch=8)
