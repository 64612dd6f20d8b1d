"""CPU tier of the HIP distillation learner (include/rl_distill.h, robot_lab_amd/distill_hip.py): header, library and binding agree, and what
the learner does not implement is refused with a reason - by the Python class and by `rl_distill_create` itself, which checks its arguments
before it touches a device (so the refusals are testable without one).  The numerics are tests/test_gpu_distill.py."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from robot_lab_amd import distill_hip
from robot_lab_amd.distill import StudentTeacher
from robot_lab_amd.distill_hip import DISTILL_EXPORTS, DistillHyper, HipDistillation
from robot_lab_amd.ppo import mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_distill.h")).read(), flags=re.S)


def test_header_library_and_binding_agree():
    declared = sorted(set(re.findall(r"\b(rl_distill_[a-z_]+)\s*\(", _header())))
    assert len(declared) >= 14
    lib = C.CDLL(distill_hip.PPO_LIB)  # the learner library: next to the PPO learner
    for name in declared:
        assert hasattr(lib, name), f"librl_ppo_hip.so does not export {name}"
    assert declared == sorted(DISTILL_EXPORTS)
    bound = distill_hip.load_distill_library()
    for name in declared:
        assert getattr(bound, name).argtypes is not None or name == "rl_distill_last_error", name


def test_hyper_struct_mirrors_the_header():
    body = re.search(r"typedef struct rl_distill_hyper \{(.*?)\}", _header(), flags=re.S).group(1)
    names = [n.strip(" *\n") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in DistillHyper._fields_]
    assert C.sizeof(DistillHyper) == 24


def test_the_ppo_header_does_not_declare_the_distillation_learner():
    src = open(os.path.join(ROOT, "include", "rl_ppo.h")).read()
    assert "rl_distill_" not in src


def test_create_refuses_before_touching_a_device():
    lib = distill_hip.load_distill_library()

    def create(dims, act=0, num_envs=64, **hyper):
        kw = dict(learning_rate=1e-3, max_grad_norm=0.0, num_learning_epochs=2, gradient_length=15, loss_type=0)
        kw.update(hyper)
        hp, n, out = DistillHyper(**kw), len(dims) - 1, C.c_void_p(0xdead)
        rc = lib.rl_distill_create((C.c_int32 * (n + 1))(*dims), n, act, C.byref(hp), num_envs, 0, C.byref(out))
        assert rc != 0 and not out.value  # a reason and a null handle
        return lib.rl_distill_last_error().decode()

    assert "activation" in create([45, 64, 12], act=1)
    assert "activation" in create([45, 64, 12], act=2)
    assert "width" in create([45, 1024, 12])
    assert "width" in create([45, 0, 12])
    assert "layer count" in create([45] * 10)
    assert "gradient_length" in create([45, 64, 12], gradient_length=0)
    assert "num_learning_epochs" in create([45, 64, 12], num_learning_epochs=0)
    for lr in (0.0, -1e-3, float("inf"), float("nan")):
        assert "learning rate" in create([45, 64, 12], learning_rate=lr)
    assert "loss type" in create([45, 64, 12], loss_type=2)
    assert "num_envs" in create([45, 64, 12], num_envs=0)
    assert "max_grad_norm" in create([45, 64, 12], max_grad_norm=-1.0)


def test_python_class_refuses_with_a_reason():
    pol = StudentTeacher(10, 14, 3, student_hidden=(32, 32), teacher_hidden=(32,))
    with pytest.raises(ValueError, match="CUDA device"):  # no CPU path and no fall-back
        HipDistillation(pol, num_envs=8)
    pol.student = mlp([10, 32, 3], activation=nn.Tanh)
    with pytest.raises(ValueError, match="unsupported activation"):
        HipDistillation(pol, num_envs=8)
    with pytest.raises(ValueError, match="width <= 512"):
        HipDistillation(StudentTeacher(10, 14, 3, student_hidden=(1024,), teacher_hidden=(32,)), num_envs=8)
    with pytest.raises(ValueError, match="loss_type"):
        HipDistillation(StudentTeacher(10, 14, 3, student_hidden=(32,), teacher_hidden=(32,)), num_envs=8, loss_type="l1")
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipDistillation(StudentTeacher(10, 14, 3, student_hidden=(32,), teacher_hidden=(32,)), num_envs=8, max_grad_norm=0.0)
