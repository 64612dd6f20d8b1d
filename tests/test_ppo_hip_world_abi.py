"""CPU tier of the HIP learner's multi-GPU split and optimiser checkpoints (include/rl_ppo.h: rl_ppo_set_world, rl_ppo_wire,
rl_ppo_update_begin, rl_ppo_minibatch_local, rl_ppo_minibatch_apply, rl_ppo_set_flat, rl_ppo_get_optimizer, rl_ppo_set_optimizer).

A handle cannot exist without a device (`rl_ppo_create` ends in hipSetDevice + hipMalloc), so the refusals of `rl_ppo_set_world` that need
a live handle (world_size < 1, a second call, a call after the first mini-batch) are exercised on the GPU in
tests/test_gpu_ppo_hip_world.py; here: the null-handle refusal of every new entry point - which also proves that each is bound with a
prototype that takes a null -, and the refusals of the Python layer, which come before the device check.  The numerics are
tests/test_gpu_ppo_hip_world.py."""
import ctypes as C
import os
import re

import pytest
import torch

from robot_lab_amd import capi, ppo_hip
from robot_lab_amd.ppo import ActorCritic
from robot_lab_amd.ppo_hip import HipPPO, adam_state_dict, adam_state_flat, parameter_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rl_ppo_set_world", "rl_ppo_wire", "rl_ppo_update_begin", "rl_ppo_minibatch_local", "rl_ppo_minibatch_apply", "rl_ppo_set_flat",
       "rl_ppo_get_optimizer", "rl_ppo_set_optimizer"]


class _Group:
    def __init__(self, world_size, enabled=True):
        self.world_size, self.enabled = world_size, enabled

    def all_reduce_sum(self, t):
        return t


def test_the_new_names_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_ppo.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rl_ppo_[a-z_]+)\s*\(", src))
    raw, bound = C.CDLL(ppo_hip.PPO_LIB), capi.load_ppo_library()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/rl_ppo.h"
        assert hasattr(raw, name), f"librl_ppo_hip.so does not export {name}"
        assert name in capi.PPO_EXPORTS
        assert getattr(bound, name).argtypes is not None, f"{name} has no prototype in the binding"


def test_every_new_entry_point_refuses_a_null_handle_with_a_reason():
    lib = capi.load_ppo_library()
    ptr, cnt, lr, step = C.c_void_p(), C.c_int64(), C.c_double(), C.c_int64()
    b = capi.Batch()
    calls = {"rl_ppo_set_world": (None, 2), "rl_ppo_wire": (None, C.byref(ptr), C.byref(cnt)), "rl_ppo_update_begin": (None, None),
             "rl_ppo_minibatch_local": (None, C.byref(b), None, 1, None), "rl_ppo_minibatch_apply": (None, None), "rl_ppo_set_flat": (None, 2, None, None),
             "rl_ppo_get_optimizer": (None, C.byref(lr), C.byref(step), None), "rl_ppo_set_optimizer": (None, 1e-3, 0, None)}
    assert sorted(calls) == sorted(NEW)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        assert b"null argument" in lib.rl_ppo_last_error(), name


def test_the_python_layer_checks_the_group_before_the_device():
    pol = ActorCritic(10, 14, 3, actor_hidden=(32,), critic_hidden=(32,))  # a CPU policy: whatever passes the group check ends at the device check
    with pytest.raises(NotImplementedError, match="torch learner"):
        HipPPO(pol, group=object())

    class NoReduce:
        world_size, enabled = 2, True

    with pytest.raises(NotImplementedError, match="all_reduce_sum"):
        HipPPO(pol, group=NoReduce())
    with pytest.raises(ValueError, match="world_size"):
        HipPPO(pol, group=_Group(0))
    for ok in (_Group(2), _Group(1, enabled=False)):
        with pytest.raises(ValueError, match="CUDA device"):  # accepted as a group; there is still no CPU path
            HipPPO(pol, group=ok)


def test_the_runner_refuses_an_unknown_learner():
    from robot_lab_amd.shims.rsl_rl.runners import learner_from_env

    assert learner_from_env({}) == "torch"
    assert learner_from_env({"RL_LEARNER": "torch"}) == "torch" and learner_from_env({"RL_LEARNER": "hip"}) == "hip"
    for bad in ("bogus", "", "HIP"):
        with pytest.raises(ValueError, match="RL_LEARNER"):
            learner_from_env({"RL_LEARNER": bad})


def test_learner_group_has_the_sum_collective():
    from robot_lab_amd.dist import LearnerGroup

    g = LearnerGroup("cpu")  # outside a launch: a world of one, every collective a no-op
    t = torch.arange(4.0)
    assert not g.enabled and g.all_reduce_sum(t) is t and torch.equal(t, torch.arange(4.0))


def test_an_optimiser_state_dict_from_fixed_arrays_loads_into_adam():
    pol = ActorCritic(19, 23, 5, actor_hidden=(40, 24), critic_hidden=(40, 24))
    shapes = parameter_shapes([19, 40, 24, 5], [23, 40, 24, 1])
    assert shapes == [tuple(p.shape) for p in pol.parameters()]
    P = sum(p.numel() for p in pol.parameters())
    m1, m2 = torch.arange(P, dtype=torch.float32) * 1e-3 - 1.0, torch.arange(P, dtype=torch.float32) * 1e-6 + 1e-4
    d = adam_state_dict(shapes, m1, m2, step=40, lr=4.4444e-4)
    opt = torch.optim.Adam(pol.parameters(), lr=1e-3)
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=1e-3)
    ref.param_groups[0]["params"][0].grad = torch.ones(2)
    ref.step()
    assert set(d["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])  # the keys of THIS torch's Adam
    assert set(d["state"][0]) == set(ref.state_dict()["state"][0]) and d["state"][0]["step"].dtype == ref.state_dict()["state"][0]["step"].dtype
    opt.load_state_dict(d)
    assert opt.param_groups[0]["lr"] == 4.4444e-4 and opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-8
    o = 0
    for p in pol.parameters():
        st = opt.state[p]
        assert float(st["step"]) == 40.0
        assert torch.equal(st["exp_avg"].reshape(-1), m1[o:o + p.numel()]) and torch.equal(st["exp_avg_sq"].reshape(-1), m2[o:o + p.numel()])
        assert st["exp_avg"].shape == p.shape
        o += p.numel()
    assert o == P
    # ... and the way back, from what torch itself writes
    b1, b2, step, lr = adam_state_flat(opt.state_dict(), shapes)
    assert torch.equal(b1, m1) and torch.equal(b2, m2) and step == 40 and lr == 4.4444e-4
    # an optimiser that has not stepped: no state either way
    fresh = adam_state_dict(shapes, torch.zeros(P), torch.zeros(P), step=0, lr=1e-3)
    assert fresh["state"] == {} and adam_state_flat(torch.optim.Adam(pol.parameters(), lr=2e-3).state_dict(), shapes) == (None, None, 0, 2e-3)
    torch.optim.Adam(pol.parameters()).load_state_dict(fresh)


def test_a_foreign_optimiser_state_is_refused_with_a_reason():
    pol = ActorCritic(19, 23, 5, actor_hidden=(40, 24), critic_hidden=(40, 24))
    shapes = parameter_shapes([19, 40, 24, 5], [23, 40, 24, 1])
    with pytest.raises(ValueError, match="defaults only"):
        adam_state_flat(torch.optim.Adam(pol.parameters(), betas=(0.8, 0.999)).state_dict(), shapes)
    with pytest.raises(ValueError, match="one param group"):
        adam_state_flat(torch.optim.Adam(list(pol.parameters())[:3]).state_dict(), shapes)
    other = ActorCritic(19, 23, 5, actor_hidden=(48, 24), critic_hidden=(40, 24))
    opt = torch.optim.Adam(other.parameters())
    sum(p.sum() for p in other.parameters()).backward()
    opt.step()
    with pytest.raises(ValueError, match="shape"):
        adam_state_flat(opt.state_dict(), shapes)
