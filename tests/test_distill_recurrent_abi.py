"""CPU tier of the recurrent distillation learner's C-ABI (include/rl_distill_bptt.h, robot_lab_amd/distill_recurrent_hip.py): header, library and
binding agree, `rl_rdistill_create` refuses what it cannot do before a device is touched, the flat layout is the order of
`StudentTeacherRecurrent.trained_parameters()`, and no other header knows the learner.  The numerics are tests/test_distill_recurrent.py (CPU)
and tests/test_gpu_distill_recurrent.py."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from robot_lab_amd import distill_recurrent_hip as rd
from robot_lab_amd.capi import PPO_LIB
from robot_lab_amd.distill_hip import DistillHyper
from robot_lab_amd.distill_recurrent import StudentTeacherRecurrent, trained_shapes
from robot_lab_amd.ppo import mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name="rl_distill_bptt.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(name="rl_distill_bptt.h"):
    return re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)


def test_header_library_and_binding_agree():
    declared = sorted(set(re.findall(r"\b(rl_rdistill_[a-z_]+)\s*\(", _code())))
    assert len(declared) == 16
    raw = C.CDLL(PPO_LIB)
    for name in declared:
        assert hasattr(raw, name), f"librl_ppo_hip.so does not export {name}"
    assert declared == sorted(rd.RDISTILL_EXPORTS)
    bound = rd.load_rdistill_library()
    src = _header()
    assert int(re.search(r"#define RL_RDISTILL_MAX_LAYERS (\d+)", src).group(1)) == rd.MAX_LAYERS == 8
    assert int(re.search(r"#define RL_RDISTILL_MAX_WIDTH (\d+)", src).group(1)) == rd.MAX_WIDTH == 512
    assert int(re.search(r"#define RL_RDISTILL_STATS (\d+)", src).group(1)) == 5
    assert '#include "rl_distill.h"' in src  # the hyper-parameters are the distillation learner's struct, not a copy
    for name in declared:  # prototypes: as many ctypes arguments as the header declares parameters
        if name == "rl_rdistill_last_error":
            continue
        params = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", _code(), flags=re.S).group(1)
        assert len(getattr(bound, name).argtypes) == params.count(",") + 1, name


def _create(obs=45, hidden=20, head=(20, 32, 12), act=0, num_envs=64, **hyper):
    lib = rd.load_rdistill_library()
    kw = dict(learning_rate=1e-3, max_grad_norm=0.0, num_learning_epochs=2, gradient_length=15, loss_type=0)
    kw.update(hyper)
    hp, n, out = DistillHyper(**kw), len(head) - 1, C.c_void_p(0xdead)
    rc = lib.rl_rdistill_create(obs, hidden, (C.c_int32 * (n + 1))(*head), n, act, C.byref(hp), num_envs, 0, C.byref(out))
    return rc, out.value, lib.rl_rdistill_last_error().decode()


@pytest.mark.parametrize("kw,reason", [
    (dict(act=1), "activation"), (dict(act=2), "activation"), (dict(obs=0), "width 0"), (dict(obs=513), "width 513"),
    (dict(hidden=513, head=(513, 8, 2)), "width 513"), (dict(hidden=0, head=(0, 8, 2)), "width 0"), (dict(head=(20, 1024, 12)), "layer width 1024"),
    (dict(head=(20, 0, 12)), "layer width 0"), (dict(head=(20,) + (8,) * 9), "layer count 9"), (dict(head=(16, 32, 12)), "hidden size"),
    (dict(gradient_length=0), "gradient_length"), (dict(num_learning_epochs=0), "num_learning_epochs"), (dict(learning_rate=0.0), "learning rate"),
    (dict(learning_rate=-1e-3), "learning rate"), (dict(learning_rate=float("inf")), "learning rate"), (dict(learning_rate=float("nan")), "learning rate"),
    (dict(loss_type=2), "loss type"), (dict(max_grad_norm=-1.0), "max_grad_norm"), (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(num_envs=0), "num_envs"), (dict(gradient_length=1 << 20, num_envs=1 << 12), "31 bits"),
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
        rd.load_rdistill_library().rl_rdistill_destroy(C.c_void_p(handle))


def test_flat_order_is_the_order_of_the_trained_parameters():
    pol = StudentTeacherRecurrent(45, 50, 12, student_hidden=(32, 16), teacher_hidden=(24,), rnn_hidden_dim=20)
    lstm = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    names = {id(p): k for k, p in pol.named_parameters()}
    trained = pol.trained_parameters()
    assert [names[id(p)] for p in trained] == [f"memory_s.rnn.{k}" for k in lstm] + [f"student.{2 * l}.{k}" for l in range(3) for k in ("weight", "bias")]
    assert trained_shapes(45, 20, [20, 32, 16, 12]) == [tuple(p.shape) for p in trained]
    assert all(p.requires_grad for p in trained) and [k for k, p in pol.named_parameters() if p.requires_grad and id(p) not in {id(q) for q in trained}] == ["std"]
    # ... and the header says so, in this order
    doc = _header()
    order = [doc.index(w) for w in ("list(memory_s.parameters()) + list(student.parameters())", "memory_s weight_ih [4H][obs]", "weight_hh [4H][H]", "bias_ih [4H]",
                                    "bias_hh [4H]; per student layer")]
    assert order == sorted(order)
    assert "0.94 GiB" in doc  # the workspace at 15 x 4096 rows, H = 256: 16 H floats per row
    assert abs(15 * 4096 * 16 * 256 * 4 / 2 ** 30 - 0.94) < 0.01


def test_other_headers_do_not_know_the_recurrent_distillation_learner():
    for h in ("rl_ppo.h", "rl_distill.h", "rl_bptt.h", "rl_lstm.h"):
        assert "rl_rdistill_" not in _header(h), h


def test_python_class_refuses_with_a_reason():
    from robot_lab_amd.distill import StudentTeacher

    make = lambda **kw: StudentTeacherRecurrent(10, 14, 3, **{**dict(student_hidden=(32,), teacher_hidden=(8,), rnn_hidden_dim=6), **kw})  # noqa: E731
    with pytest.raises(TypeError, match="StudentTeacherRecurrent"):
        rd.HipRecurrentDistillation(StudentTeacher(10, 14, 3, student_hidden=(32,), teacher_hidden=(8,)), num_envs=8)
    with pytest.raises(ValueError, match="CUDA device"):  # no CPU path and no fall-back
        rd.HipRecurrentDistillation(make(), num_envs=8)
    pol = make()
    pol.student = mlp([6, 32, 3], activation=nn.Tanh)
    with pytest.raises(ValueError, match="unsupported activation"):
        rd.HipRecurrentDistillation(pol, num_envs=8)
    with pytest.raises(ValueError, match="width <= 512"):
        rd.HipRecurrentDistillation(make(student_hidden=(1024,)), num_envs=8)
    with pytest.raises(ValueError, match="loss_type"):
        rd.HipRecurrentDistillation(make(), num_envs=8, loss_type="l1")
    with pytest.raises(ValueError, match="max_grad_norm"):
        rd.HipRecurrentDistillation(make(), num_envs=8, max_grad_norm=0.0)
