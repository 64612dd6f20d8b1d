"""`-m gpu`: the HIP PPO learner on every branch of its loss head (`ppo_head_kernel`) and through the clipped Adam step (`ppo_sumsq_kernel`,
`ppo_adam_kernel`: gradient norm, clip coefficient, moments, the floor of std), against the unchanged `ppo.PPO` in fp64.

The batch the other learner tests share stays on ONE path of the head (ratio inside the band, no value clipped: tests/test_ppo.py pins that down)
and Adam hides the scale of the gradient, so here the batch is designed (`ppo_helpers.branch_storage`): old log-probs, old values and returns are
set from the fp64 forward so that every row's branch is fixed by construction, >= 10 % of the rows in each outcome and no row within 0.01 of a
switch - 1e4 x the distance between the HIP forward and fp64, so the two sides cannot disagree on a branch; nothing is masked.  tests/test_ppo.py
checks the batch on the CPU and shows that each of six wrong head rules moves some tensor's gradient by >= 100 x the bound used here.

Comparator and bounds as in tests/test_gpu_ppo_hip.py: `ppo.PPO` in fp64 from the same parameters, `ppo.PPO` in fp32 beside it for d; gradients
and Adam moments e <= max(8 d, floor) per parameter tensor (`ppo_helpers.compare_gradients`), statistics |hip - f64| <= 8 |f32 - f64| + 1e-6 |f64|,
parameters q999 <= max(8 q999_32, ulp) and max <= the sum of the learning rates.  Shapes (`ppo_helpers.BRANCH_SHAPES`): the A1 network on 1000
rows with a handle created for 1536 (row tails of every tile, the head's tail block, empty dW chunks) and ActorCritic(19, 23, 5, hidden (40, 24))
on 37 rows.  The tables are profiles/ppo_hip_branch_parity.txt."""
import copy
import functools

import numpy as np
import pytest

from ppo_helpers import (BRANCH_SHAPES, DEV, branch_case, branch_classes, branch_storage, cast as _cast, check_branches, compare_gradients, gen as _gen,
                         reference_gradients, split as _split, tables, torch_learner as _torch_learner)

pytestmark = pytest.mark.gpu

SHAPES = list(BRANCH_SHAPES)
MAX_ROWS = {"a1-1000": 1536, "odd-37": 37}
ONE_STEP = dict(num_learning_epochs=1, num_mini_batches=1, schedule="fixed")


@functools.lru_cache(maxsize=None)
def _reference(shape, clipped=True):
    """the references' gradients on the designed batch, computed once per shape and rule and read-only; with them the gradient norm as fp64 has it
    and as the fp32 torch learner computes it (`clip_grad_norm_` on its gradients, which it left unscaled)"""
    import torch

    pol, st, _ = branch_case(shape)
    ref, algs = reference_gradients(pol, st, use_clipped_value_loss=clipped)
    norm = {dtype: float(torch.nn.utils.clip_grad_norm_(alg.policy.parameters(), 1e30)) for dtype, alg in algs.items()}
    return ref, norm


def _hip(pol, shape, **kw):
    from robot_lab_amd.ppo_hip import HipPPO

    return HipPPO(copy.deepcopy(pol).to(DEV), max_rows_per_minibatch=MAX_ROWS[shape], **kw)


def _named(alg, what=None):
    """{parameter name: the parameter, or entry `what` of its Adam state; fp64 on the host}"""
    return {n: (p if what is None else alg.optimizer.state[p][what]).detach().double().cpu() for n, p in alg.policy.named_parameters()}


def _parameters_off(title, ph, p64, p32, displacement):
    """the parameter rule of test_gpu_ppo_hip.py::test_one_update_matches_the_torch_learner: prints the table, returns what breaks it"""
    import torch

    print(f"\n{title}\n{'tensor':<18}{'q999 hip':>12}{'q999 torch32':>14}{'max hip':>12}{'max torch32':>13}")
    bad = []
    for n in p64:
        dh, d32 = (ph[n].reshape(p64[n].shape) - p64[n]).abs().flatten(), (p32[n] - p64[n]).abs().flatten()
        qh, q32 = torch.quantile(dh, 0.999).item(), torch.quantile(d32, 0.999).item()
        ulp = float(np.spacing(np.float32(p64[n].abs().max().item())))
        print(f"{n:<18}{qh:12.3e}{q32:14.3e}{dh.max().item():12.3e}{d32.max().item():13.3e}")
        if not qh <= max(8 * q32, ulp):
            bad.append((n, "q999", qh, q32))
        if not dh.max().item() <= displacement:
            bad.append((n, "max", dh.max().item(), displacement))
    return bad


@pytest.mark.parametrize("clipped", [True, False], ids=["clipped-value-loss", "plain-value-loss"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_parity_on_every_branch(shape, clipped):
    """e <= max(8 d, floor) per parameter tensor where every outcome of the surrogate (tie, t1 > t2, t1 < t2 with a zero gradient, adv == 0) and of
    the value loss (in-band, l1 > l2, l1 < l2 for either sign of dv) carries rows; `use_clipped_value_loss=False` on both sides: the other head path"""
    import torch

    pol, st, cls = branch_case(shape)
    check_branches(shape, cls)
    ref, _ = _reference(shape, clipped)
    hip = _hip(pol, shape, use_clipped_value_loss=clipped)
    g_hip = _split(hip.minibatch_grad(_cast(st, torch.float32), torch.arange(cls.rows, device=DEV)), pol)
    torch.cuda.synchronize()
    bad = compare_gradients(f"{shape}, use_clipped_value_loss={clipped}: gradients", g_hip, ref)
    hip.close()
    assert not bad, f"gradient error above max(8 x the fp32 torch learner's, floor): {bad}"


@pytest.mark.parametrize("schedule", ["fixed", "adaptive"])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_statistics_of_one_minibatch(shape, schedule):
    """value_loss and surrogate_loss of one mini-batch - sums over clipped and unclipped rows - and, under the adaptive schedule, the KL statistic
    and the learning rate it leads to"""
    import torch

    pol, st, _ = branch_case(shape)
    kw = dict(ONE_STEP, schedule=schedule)
    a64, a32 = _torch_learner(pol, torch.float64, **kw), _torch_learner(pol, torch.float32, **kw)
    s64, s32 = a64.update(_cast(st, torch.float64), _gen()), a32.update(_cast(st, torch.float32), _gen())
    hip = _hip(pol, shape, **kw)
    s_hip = hip.update(_cast(st, torch.float32), _gen())
    hip.close()
    print(f"\n{shape}, {schedule}: statistic (hip, torch32, torch64) " + ", ".join(f"{k} ({s_hip[k]:.9g}, {s32[k]:.9g}, {s64[k]:.9g})" for k in s64))
    assert s64["value_loss"] > 0 and s64["surrogate_loss"] != 0 and (s64["kl"] > 0.04) == (schedule == "adaptive")  # (thresholds 0.02, 0.005)
    for k in ("value_loss", "surrogate_loss", "entropy", "kl"):
        assert abs(s_hip[k] - s64[k]) <= 8 * abs(s32[k] - s64[k]) + 1e-6 * abs(s64[k]), (k, s_hip[k], s32[k], s64[k])
    assert s_hip["learning_rate"] == s64["learning_rate"] == s32["learning_rate"]
    assert (s64["learning_rate"] != 1e-3) == (schedule == "adaptive"), "the KL of the designed batch was meant to move the learning rate"


def test_gradient_parity_on_every_branch_with_symmetry():
    """the same through the `SYM` head with the augmentation on: a virtual row reads its stored terms through its stored row, so the copy-1 rows
    take whatever branch the mirrored forward gives them (margins checked in fp64, here and in tests/test_ppo.py); reference: `PPO(symmetry=...)`"""
    import torch

    shape = "odd-37"
    pol, st, _ = branch_case(shape)
    tab = tables(BRANCH_SHAPES[shape]["dims"], n_sym=2)
    c = branch_classes(pol, st, symmetry=tab)
    check_branches(f"{shape} x 2 copies", c, share=None)
    assert len(set(c.sur.tolist())) == 3 and len(set(c.val.tolist())) == 5
    ref, _ = reference_gradients(pol, st, symmetry=tab)
    hip = _hip(pol, shape, symmetry=tab)
    g_hip = _split(hip.minibatch_grad(_cast(st, torch.float32), torch.arange(c.rows // 2, device=DEV)), pol)
    torch.cuda.synchronize()
    bad = compare_gradients(f"{shape} x 2 copies: gradients", g_hip, ref)
    hip.close()
    assert not bad, f"gradient error above max(8 x the fp32 torch learner's, floor): {bad}"


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_norm_clip_coefficient_and_moments(shape):
    """one optimiser step from zero moments with max_grad_norm = norm64 / 2 (coef = 1 / 2) and 2 norm64 (coef = 1), a factor 2 either side of the
    threshold: the norm the learner reports, and exp_avg = 0.1 coef g, exp_avg_sq = 0.001 (coef g)^2 per tensor against the fp64 learner's Adam
    state.  Adam's step hides the scale of g; the moments do not: a missing coef is a factor 2 in exp_avg and 4 in exp_avg_sq."""
    import torch

    pol, st, _ = branch_case(shape)
    _, norm = _reference(shape)
    n64, n32 = norm[torch.float64], norm[torch.float32]
    bad, m_hip = [], {}
    for factor in (0.5, 2.0):
        kw = dict(ONE_STEP, max_grad_norm=factor * n64)
        algs = {dtype: _torch_learner(pol, dtype, **kw) for dtype in (torch.float64, torch.float32)}
        for dtype, alg in algs.items():
            alg.update(_cast(st, dtype), _gen())
        hip = _hip(pol, shape, **kw)
        hip.update(_cast(st, torch.float32), _gen())
        print(f"\n{shape}, max_grad_norm = {factor} norm64: gradient norm hip {hip.last_grad_norm:.9g}, torch32 {n32:.9g}, torch64 {n64:.9g}")
        if not abs(hip.last_grad_norm - n64) <= 8 * abs(n32 - n64) + 1e-6 * n64:
            bad.append(("norm", factor, hip.last_grad_norm, n32, n64))
        for what in ("exp_avg", "exp_avg_sq"):
            m_hip[what, factor] = hip.flat(what)
            ref = {dtype: _named(alg, what) for dtype, alg in algs.items()}
            bad += [(what, factor) + b for b in compare_gradients(f"{shape}, max_grad_norm = {factor} norm64: {what}", _split(m_hip[what, factor], pol), ref)]
        hip.close()
    for what, power in (("exp_avg", 1), ("exp_avg_sq", 2)):
        lo, hi = m_hip[what, 0.5].double(), m_hip[what, 2.0].double()
        k = int(hi.abs().argmax())
        print(f"{shape}: {what} of the clipped step / of the unclipped one, at the largest entry: {float(lo[k] / hi[k]):.7f} (0.5 ** {power} = {0.5 ** power})")
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES)
def test_clip_coefficient_reaches_the_parameters_in_the_second_step(shape):
    """two consecutive steps, the first clipped by two and the second not: the second step divides moments that mix a scaled and an unscaled
    gradient, so here - and not after one step - the coefficient moves the parameters (3.5 % of a step where the two gradients are alike).  The
    HIP learner's clipping norm belongs to its handle: the second step runs on a second handle that resumes the first one's checkpoint."""
    import torch

    pol, st, _ = branch_case(shape)
    _, norm = _reference(shape)
    first = norm[torch.float64] / 2

    def two_steps(dtype, second):
        alg = _torch_learner(pol, dtype, **dict(ONE_STEP, max_grad_norm=first))
        alg.update(_cast(st, dtype), _gen(1))
        alg.max_grad_norm = second
        alg.update(_cast(st, dtype), _gen(2))
        return alg

    probe = two_steps(torch.float64, 1e30)  # (its second step left its gradients unscaled)
    second = 2 * float(torch.nn.utils.clip_grad_norm_(probe.policy.parameters(), 1e30))
    a64, a32 = two_steps(torch.float64, second), two_steps(torch.float32, second)
    st32 = _cast(st, torch.float32)
    one = _hip(pol, shape, **dict(ONE_STEP, max_grad_norm=first))
    one.update(st32, _gen(1))
    two = _hip(one.store_into(copy.deepcopy(pol).to(DEV)), shape, **dict(ONE_STEP, max_grad_norm=second))
    two.load_optimizer_state_dict(one.optimizer_state_dict())
    two.update(st32, _gen(2))
    ph = _split(two.flat("parameters"), pol)
    torch.cuda.synchronize()
    print(f"\n{shape}: clipping norms {first:.6g}, {second:.6g}; gradient norms of the HIP learner {one.last_grad_norm:.6g}, {two.last_grad_norm:.6g}")
    assert one.last_grad_norm > 1.9 * first and two.last_grad_norm < 0.6 * second
    bad = _parameters_off(f"{shape}: parameters after a clipped and an unclipped step", ph, _named(a64), _named(a32), displacement=float(sum(a64.lr_path)))
    one.close(); two.close()
    assert not bad, bad


def test_floor_of_std():
    """std = 5e-4 and one step of 1e-2: an entry of std whose gradient is positive would land at -9.5e-3 and is floored, one whose gradient is negative
    rises to 1.05e-2.  Where the fp64 learner floors, the HIP parameter is exactly 1e-6f; the rest follows the parameter rule; all finite.  The
    storage is designed from this policy, so (a - mu) / sigma stays O(1) and every log-density is finite."""
    import torch

    from robot_lab_amd.ppo import ActorCritic

    shape = "odd-37"
    s = BRANCH_SHAPES[shape]
    torch.manual_seed(0)
    pol = ActorCritic(*s["dims"], actor_hidden=s["hidden"], critic_hidden=s["hidden"], init_noise_std=5e-4)
    st, cls = branch_storage(pol, s["rows"], *s["dims"], seed=s["seed"])
    check_branches(f"{shape}, std 5e-4", cls)
    kw = dict(ONE_STEP, learning_rate=1e-2)
    algs, before = {}, {}
    for dtype in (torch.float64, torch.float32):
        alg = algs[dtype] = _torch_learner(pol, dtype, **kw)
        step = alg.optimizer.step

        def recording_step(*a, alg=alg, step=step, dtype=dtype, **k):
            out = step(*a, **k)
            before[dtype] = alg.policy.std.detach().double().cpu().clone()  # after Adam, before the floor
            return out

        alg.optimizer.step = recording_step
        alg.update(_cast(st, dtype), _gen())
    pre = before[torch.float64]
    floored = pre < -1e-3
    print(f"\n{shape}: std of the fp64 learner after Adam, before the floor: {pre.tolist()}")
    assert bool(floored.any()) and bool((pre[~floored] > 1e-3).all()) and not bool(floored.all()), "the batch was meant to floor some entries of std and raise others"
    hip = _hip(pol, shape, **kw)
    hip.update(_cast(st, torch.float32), _gen())
    flat = hip.flat("parameters")
    ph = _split(flat, pol)
    torch.cuda.synchronize()
    print(f"{shape}: std of the HIP learner {ph['std'].tolist()}")
    assert bool(torch.isfinite(flat).all())
    assert bool((ph["std"][floored].float() == torch.tensor(1e-6, dtype=torch.float32)).all()), "a floored entry of std is not exactly 1e-6f"
    assert bool((ph["std"][~floored] > 1e-3).all())
    bad = _parameters_off(f"{shape}: parameters after the step that floors std", ph, _named(algs[torch.float64]), _named(algs[torch.float32]), displacement=1e-2)
    hip.close()
    assert not bad, bad
