"""The one copy of what the distillation tests share (tests/test_distill.py on the CPU, tests/test_gpu_distill.py on the GPU): the exact integer
family and its int64 gradients, a float batch for the fp64-referenced bound, and the torch rule run with its optimiser steps recorded.
`torch` is imported inside the functions: the module imports wherever its users do."""
import copy
import functools
import types

import numpy as np

# the exact family: one-layer student 45 -> 8, N = 128 (N A = 2^10), integer observations in [-3, 3], weights in [-2, 2], teacher actions in [-4, 4], zero bias
EX = dict(obs=45, A=8, N=128, T=5, gradient_length=3, epochs=2)


@functools.lru_cache(maxsize=None)
def exact_family(seed=0):
    """(W [8, 45] int64, obs [T, N, 45] int64, teacher actions [T, N, 8] int64); read-only"""
    rng = np.random.default_rng(seed)
    W = rng.integers(-2, 3, size=(EX["A"], EX["obs"]))
    obs = rng.integers(-3, 4, size=(EX["T"], EX["N"], EX["obs"]))
    ta = rng.integers(-4, 5, size=(EX["T"], EX["N"], EX["A"]))
    return W.astype(np.int64), obs.astype(np.int64), ta.astype(np.int64)


def exact_group_sums(steps, seed=0):
    """(sum over the rows of the listed steps of d x^T [8, 45], of d [8]) in int64, d = W x - a*; asserts that every partial sum a fp32 GEMM can
    form is exact: |sum d x| <= rows * 274 * 3 < 2^24 for the 384 rows of a full group"""
    W, obs, ta = exact_family(seed)
    x = np.concatenate([obs[t] for t in steps], 0)
    a = np.concatenate([ta[t] for t in steps], 0)
    d = x @ W.T - a
    assert np.abs(x @ W.T).max() <= 45 * 2 * 3 and np.abs(d).max() <= 274
    assert len(steps) * EX["N"] <= 512 and 384 * 274 * 3 < 512 * 274 * 3 < 2 ** 24  # (a full group has 384 rows; a defective one of the tests up to 512)
    assert (np.abs(d)[:, :, None] * np.abs(x)[:, None, :]).sum(0).max() < 2 ** 24  # every partial sum, in any order
    return d.T @ x, d.sum(0)


def exact_group_gradient(steps, seed=0, shift=-9):
    """the flat fp32 gradient (W, then b) of sum over the steps of the MSE means: the int64 sums times 2 / (N A) = 2^-9"""
    gw, gb = exact_group_sums(steps, seed)
    return np.concatenate([np.ldexp(gw.astype(np.float64), shift).reshape(-1), np.ldexp(gb.astype(np.float64), shift)]).astype(np.float32)


def exact_policy(seed=0, device="cpu"):
    """a StudentTeacher whose student is the family's layer (no hidden layer, zero bias), and the float batch"""
    import torch

    from robot_lab_amd.distill import StudentTeacher

    W, obs, ta = exact_family(seed)
    pol = StudentTeacher(EX["obs"], EX["obs"], EX["A"], student_hidden=(), teacher_hidden=(16,), init_noise_std=0.1)
    with torch.no_grad():
        pol.student[0].weight.copy_(torch.as_tensor(W, dtype=torch.float32))
        pol.student[0].bias.zero_()
    batch = types.SimpleNamespace(observations=torch.as_tensor(obs, dtype=torch.float32).to(device), teacher_actions=torch.as_tensor(ta, dtype=torch.float32).to(device))
    return pol.to(device), batch


def recorded_update(alg, batch, step=True):
    """`alg.update(batch)` of a torch `Distillation` with every optimiser step recorded: returns (result, [flat student gradient per step, fp64 on
    the host], [flat student parameters after each step]).  `step=False`: the parameters are NOT moved (the gradients of frozen parameters)."""
    import torch

    grads, params = [], []
    real = alg.optimizer.step
    student = alg.policy.student

    def recording(*a, **k):
        grads.append(torch.cat([p.grad.detach().reshape(-1) for p in student.parameters()]).double().cpu())
        out = real(*a, **k) if step else None
        params.append(torch.cat([p.detach().reshape(-1) for p in student.parameters()]).double().cpu())
        return out

    alg.optimizer.step = recording
    try:
        res = alg.update(batch)
    finally:
        alg.optimizer.step = real
    return res, grads, params


# ---- the float cases of the fp64-referenced bound
SHAPES = {"ragged": dict(obs=45, hidden=(64, 32), A=12, N=130, T=5, gradient_length=3, epochs=2),
          "tiles": dict(obs=45, hidden=(128, 128, 128), A=12, N=256, T=4, gradient_length=2, epochs=2)}


@functools.lru_cache(maxsize=None)
def float_case(name, huber=False):
    """(StudentTeacher on the host in fp32, batch on the host in fp32) of SHAPES[name]; the teacher actions are the teacher's own on the rows plus
    noise.  `huber`: the teacher actions are scaled and moved so that, in fp64, at least 10 % of the entries of d = student - teacher sit on
    either side of |d| = 1 and none within 0.01 of it (asserted)."""
    import torch

    from robot_lab_amd.distill import StudentTeacher

    s = SHAPES[name]
    torch.manual_seed(3)
    pol = StudentTeacher(s["obs"], s["obs"], s["A"], student_hidden=s["hidden"], teacher_hidden=(32,), init_noise_std=0.1)
    g = torch.Generator().manual_seed(7)
    obs = torch.randn(s["T"], s["N"], s["obs"], generator=g)
    with torch.no_grad():
        ta = pol.teacher(obs) + 0.3 * torch.randn(s["T"], s["N"], s["A"], generator=g)
        if huber:
            p64 = copy.deepcopy(pol).double()
            mu = p64.student(obs.double())
            ta = ta.double() * 3.0
            d = mu - ta
            near = (d.abs() - 1.0).abs() < 0.02
            ta = torch.where(near, ta + 0.05 * torch.sign(d) * torch.where(d.abs() >= 1.0, -1.0, 1.0), ta).float()  # away from the switch, to its own side
            d = mu - ta.double()
            inside = float((d.abs() < 1.0).double().mean())
            assert inside >= 0.10 and 1.0 - inside >= 0.10, inside
            assert float((d.abs() - 1.0).abs().min()) >= 0.01
    return pol, types.SimpleNamespace(observations=obs.contiguous(), teacher_actions=ta.float().contiguous())


def cast_case(pol, batch, dtype, device):
    import torch

    p = copy.deepcopy(pol).to(device=device, dtype=dtype)
    b = types.SimpleNamespace(observations=batch.observations.to(device=device, dtype=dtype), teacher_actions=batch.teacher_actions.to(device=device, dtype=dtype))
    return p, b


def split_student(flat, pol):
    """{student parameter name: its slice of the flat buffer, fp64 on the host}"""
    out, o = {}, 0
    for name, p in pol.student.named_parameters():
        out[name] = flat[o:o + p.numel()].double().cpu().reshape(p.shape)
        o += p.numel()
    assert o == flat.numel()
    return out


def within_bound(title, got, ref64, ref32, lines=None):
    """per tensor: e = max|got - ref64| / max|ref64| against d = max|ref32 - ref64| / max|ref64|; the bound is e <= 8 d.  Prints (and appends to
    `lines`) the measured multiples, with one fp32 spacing of max|ref64| relative to it for scale (`floor`, not part of the bound); returns the
    tensors above the bound."""
    bad = []
    for n, r64 in ref64.items():
        scale = float(np.abs(np.asarray(r64, dtype=np.float64)).max())
        assert scale > 0, n
        e = float(np.abs(np.asarray(got[n], dtype=np.float64) - np.asarray(r64, dtype=np.float64)).max()) / scale
        d = float(np.abs(np.asarray(ref32[n], dtype=np.float64) - np.asarray(r64, dtype=np.float64)).max()) / scale
        floor = float(np.spacing(np.float32(scale))) / scale
        line = f"{title:<44}{n:<12}{scale:12.4e}{e:12.3e}{d:12.3e}{(e / d if d else float('inf')):8.2f}{floor:12.3e}"
        print(line)
        if lines is not None:
            lines.append(line)
        if not e <= 8 * d:
            bad.append((title, n, e, d, floor))
    return bad
