"""CPU tier of the HIP PPO learner (include/rl_ppo.h, robot_lab_amd/ppo_hip.py): header, library and binding agree, and what the learner
does not implement is refused with a reason - by the Python class and by `rl_ppo_create` itself, which checks its arguments before it
touches a device (so the refusals are testable without one).  The numerics are tests/test_gpu_ppo_hip.py."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from robot_lab_amd import ppo_hip
from robot_lab_amd.ppo import ActorCritic, mlp
from robot_lab_amd.ppo_hip import HipPPO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header, prefix):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree():
    declared = _declared("rl_ppo.h", "rl_ppo_")
    assert len(declared) >= 8
    lib = C.CDLL(ppo_hip.PPO_LIB)
    for name in declared:
        assert hasattr(lib, name), f"librl_ppo_hip.so does not export {name}"
    assert declared == sorted(ppo_hip.PPO_EXPORTS)
    bound = ppo_hip.load_ppo_library()
    for name in declared:  # every entry point has a prototype in the binding (restype-only ones aside)
        assert getattr(bound, name).argtypes is not None or name == "rl_ppo_last_error", name


def test_device_push_is_declared_exported_and_bound():
    from robot_lab_amd.policy import POLICY_EXPORTS, POLICY_LIB, MlpPolicy

    assert "rl_mlp_set_weights_device" in _declared("rl_policy.h", "rl_mlp_")
    assert hasattr(C.CDLL(POLICY_LIB), "rl_mlp_set_weights_device")
    assert "rl_mlp_set_weights_device" in POLICY_EXPORTS and hasattr(MlpPolicy, "set_weights_device")


def test_hyper_struct_mirrors_the_header():
    """field order of `rl_ppo_hyper` / `rl_ppo_batch` in the header = the ctypes mirrors"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_ppo.h")).read(), flags=re.S)
    body = re.search(r"typedef struct rl_ppo_hyper \{(.*?)\}", src, flags=re.S).group(1)
    names = [n.strip(" *\n") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in ppo_hip.Hyper._fields_]
    body = re.search(r"typedef struct rl_ppo_batch \{(.*?)\}", src, flags=re.S).group(1)
    names = [n.strip(" *\n") for decl in body.split(";") if decl.strip() for n in decl.replace("const float", "").split(",")]
    assert names == [f[0] for f in ppo_hip.Batch._fields_]
    assert C.sizeof(ppo_hip.Hyper) == 56


def test_group_is_refused_naming_the_torch_learner():
    with pytest.raises(NotImplementedError, match="torch learner"):
        HipPPO(ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,)), group=object())


def test_unsupported_networks_are_refused_with_a_reason():
    pol = ActorCritic(10, 14, 3, actor_hidden=(32, 32), critic_hidden=(32, 32))
    pol.actor = mlp([10, 32, 32, 3], activation=nn.Tanh)
    with pytest.raises(ValueError, match="unsupported activation"):
        HipPPO(pol)
    pol = ActorCritic(10, 14, 3, actor_hidden=(32, 32), critic_hidden=(32,))
    with pytest.raises(ValueError, match="differ in depth"):
        HipPPO(pol)
    pol = ActorCritic(10, 14, 3, actor_hidden=(1024,), critic_hidden=(32,))
    with pytest.raises(ValueError, match="width <= 512"):
        HipPPO(pol)
    pol = ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,))
    pol.noise_std_type = "log"
    with pytest.raises(ValueError, match="noise_std_type"):
        HipPPO(pol)
    with pytest.raises(ValueError, match="schedule"):
        HipPPO(ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,)), schedule="linear")


def test_create_refuses_before_touching_a_device():
    lib = ppo_hip.load_ppo_library()

    def create(adims, cdims, act=0, **hyper):
        kw = dict(learning_rate=1e-3, desired_kl=0.01, value_loss_coef=1.0, clip_param=0.2, entropy_coef=0.01, max_grad_norm=1.0, use_clipped_value_loss=1,
                  num_learning_epochs=5, num_mini_batches=4, schedule=1, std_type=0)
        kw.update(hyper)
        hp, n, out = ppo_hip.Hyper(**kw), len(adims) - 1, C.c_void_p()
        rc = lib.rl_ppo_create((C.c_int32 * (n + 1))(*adims), (C.c_int32 * (n + 1))(*cdims), n, act, C.byref(hp), 1024, 0, C.byref(out))
        assert rc != 0 and not out.value
        return lib.rl_ppo_last_error().decode()

    assert "activation" in create([45, 64, 12], [235, 64, 1], act=2)
    assert "noise_std_type" in create([45, 64, 12], [235, 64, 1], std_type=1)
    assert "width" in create([45, 1024, 12], [235, 64, 1])
    assert "critic" in create([45, 64, 12], [235, 64, 2])
    assert "layer count" in create([45] * 10, [235] * 10)
    assert "desired_kl" in create([45, 64, 12], [235, 64, 1], desired_kl=0.0)


def test_trainer_keeps_the_torch_learner_by_default():
    import inspect

    from robot_lab_amd.ppo import Trainer

    sig = inspect.signature(Trainer.__init__)
    assert sig.parameters["learner"].default == "torch"


def test_a_cpu_policy_is_refused_not_routed_elsewhere():
    """no CPU path and no fall-back: a policy that is not on a CUDA device is refused by name, before the library is touched"""
    with pytest.raises(ValueError, match="CUDA device"):
        HipPPO(ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,)))


def test_desired_kl_must_be_positive_or_none():
    """`ppo.PPO` with desired_kl = 0.0 lowers the learning rate at every positive KL: a degenerate rule the HIP learner refuses instead of
    reinterpreting (None = no adaptive schedule, as in ppo.py)"""
    for bad in (0.0, -0.01):
        with pytest.raises(ValueError, match="desired_kl"):
            HipPPO(ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,)), desired_kl=bad)


def test_the_binding_lives_in_capi():
    from robot_lab_amd import capi

    assert capi.PPO_EXPORTS is ppo_hip.PPO_EXPORTS and capi.load_ppo_library is ppo_hip.load_ppo_library
