"""`-m gpu`: the HIP learner's mini-batch split around a caller's all-reduce (rl_ppo_set_world, rl_ppo_update_begin, rl_ppo_minibatch_local,
rl_ppo_minibatch_apply, the wire) and its optimiser checkpoints, in ONE process without torch.distributed: the group is a stub whose
`all_reduce_sum` does to the wire what a SUM over `world_size` identical ranks does.

  world 1, identity    begin + n x (local, apply) must be rl_ppo_update bit for bit
  world 2, t + t       x + x and / 2 are exact in fp32: bit-identical to the single learner, INCLUDING the gradient norm and the KL statistic - Adam
                       is invariant to the scale of the gradient, so the parameters alone would hide a forgotten / world; these two would not
  world 3, 3 t         fl(fl(3 g) / 3) is within 1 ulp of g: norm and KL within 1e-6 relative, and the parameters against the unchanged `ppo.PPO` in
                       fp64 with the equivalent stub (x 3, / 3), inside 8 x the fp32 torch learner's own distance from it - the comparator, the
                       method and the bound of tests/test_gpu_ppo_hip.py::test_one_update_matches_the_torch_learner

Synthetic storage as in tests/test_gpu_ppo_hip.py at small odd shapes: ActorCritic(19, 23, 5, hidden (40, 24)), T = 4, N = 37: 148 rows,
mini-batches of 37 (row tails of every tile, a partial 16-row slice, empty dW chunks), 2 epochs x 4 mini-batches, parameters perturbed by
0.01 randn mean|p|.  The single learner's update is computed once (fixture `single`) and shared."""
import copy
import ctypes as C

import numpy as np
import pytest

from ppo_helpers import DEV, cast as _cast, fake_storage as _fake_storage, gen as _gen

pytestmark = pytest.mark.gpu

T, N, OD, CD, A = 4, 37, 19, 23, 5
HID = (40, 24)
B, NMB, EPOCHS = T * N, 4, 2
MB = B // NMB
KW = dict(num_learning_epochs=EPOCHS, num_mini_batches=NMB)


class _Ranks:
    """`world_size` identical ranks: the SUM all-reduce of the wire is a multiplication"""

    enabled = True

    def __init__(self, world_size):
        self.world_size, self.calls, self.sizes = world_size, 0, set()

    def all_reduce_sum(self, t):
        self.calls += 1
        self.sizes.add(t.numel())
        if self.world_size == 2:
            t.add_(t)
        elif self.world_size > 2:
            t.mul_(self.world_size)
        return t


class _TorchRanks:
    """the same world for `ppo.PPO` (dist.LearnerGroup's `mean` and `reduce_gradients`: SUM, then / world)"""

    def __init__(self, world_size):
        self.world_size = world_size

    def mean(self, value):
        t = value.detach().clone().reshape(1)
        t.mul_(self.world_size)
        return (t / self.world_size).reshape(())

    def reduce_gradients(self, module):
        for p in module.parameters():
            if p.grad is not None:
                p.grad.mul_(self.world_size)
                p.grad.div_(self.world_size)


@pytest.fixture(scope="module")
def case():
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pol = ActorCritic(OD, CD, A, actor_hidden=HID, critic_hidden=HID)
    st = _fake_storage(pol, T, N, OD, CD, A)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g) * p.abs().mean())
    return pol, st, _cast(st, torch.float32)


def _hip(pol, **kw):
    from robot_lab_amd.ppo_hip import HipPPO

    return HipPPO(copy.deepcopy(pol).to(DEV), **dict(KW, **kw))


def _optimizer(hip):
    lr, step = C.c_double(), C.c_int64()
    assert hip.lib.rl_ppo_get_optimizer(hip.handle, C.byref(lr), C.byref(step), hip._stream()) == 0
    return lr.value, step.value


def _snap(hip, stats):
    lr, step = _optimizer(hip)
    return dict(p=hip.flat("parameters").cpu(), m1=hip.flat("exp_avg").cpu(), m2=hip.flat("exp_avg_sq").cpu(), lr=lr, step=step, stats=dict(stats),
                norm=hip.last_grad_norm)


def _update(pol, st32, **kw):
    hip = _hip(pol, **kw)
    snap = _snap(hip, hip.update(st32, _gen()))
    hip.close()
    return snap


@pytest.fixture(scope="module")
def single(case):
    """one update of the learner on its own (rl_ppo_update): the reference of the bit-identity tests"""
    pol, _, st32 = case
    s = _update(pol, st32)
    assert s["step"] == EPOCHS * NMB and s["stats"]["kl"] > 0 and s["norm"] > 0 and bool(s["m2"].max() > 0)
    return s


def _same_state(a, b):
    import torch

    for k in ("p", "m1", "m2"):
        assert torch.equal(a[k], b[k]), f"{k} differs: max |d| {(a[k] - b[k]).abs().max().item():.3e}"
    assert a["lr"] == b["lr"] and a["step"] == b["step"]


def test_split_equals_fused(case, single):
    pol, _, st32 = case
    g = _Ranks(1)
    s = _update(pol, st32, group=g)
    assert g.calls == EPOCHS * NMB and g.sizes == {single["p"].numel() + 1}  # one collective per mini-batch, P + 1 words
    _same_state(s, single)
    assert s["stats"] == single["stats"] and s["norm"] == single["norm"]


def test_two_identical_ranks_equal_one(case, single):
    pol, _, st32 = case
    s = _update(pol, st32, group=_Ranks(2))
    _same_state(s, single)
    print(f"\nnorm {s['norm']!r} / {single['norm']!r}  kl {s['stats']['kl']!r} / {single['stats']['kl']!r}")
    assert s["norm"] == single["norm"], "the gradient norm is not that of g / world"
    assert s["stats"]["kl"] == single["stats"]["kl"], "the KL statistic is not the ranks' mean"
    assert s["stats"] == single["stats"]


def test_three_identical_ranks(case, single):
    import torch

    from robot_lab_amd.ppo import PPO

    pol, st, st32 = case
    s = _update(pol, st32, group=_Ranks(3))
    print(f"\nnorm {s['norm']!r} / {single['norm']!r}  kl {s['stats']['kl']!r} / {single['stats']['kl']!r}  lr {s['lr']!r} / {single['lr']!r}")
    assert abs(s["norm"] - single["norm"]) <= 1e-6 * abs(single["norm"])
    assert abs(s["stats"]["kl"] - single["stats"]["kl"]) <= 1e-6 * abs(single["stats"]["kl"])
    assert s["lr"] == single["lr"] and s["step"] == single["step"]
    # the parameters: `ppo.PPO` in fp64 with the equivalent stub, and in fp32 as the measure of what fp32 round-off alone does
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = PPO(copy.deepcopy(pol).to(device=DEV, dtype=dtype), group=_TorchRanks(3), **KW)
        alg.lr_path = []
        step = alg.optimizer.step

        def recording_step(*a, _alg=alg, _step=step, **k):
            _alg.lr_path.append(_alg.optimizer.param_groups[0]["lr"])
            return _step(*a, **k)

        alg.optimizer.step = recording_step
        stats = alg.update(_cast(st, dtype), _gen())
        ref[dtype] = (alg, stats, {n: p.detach().double().cpu() for n, p in alg.policy.named_parameters()})
    a64, s64, p64 = ref[torch.float64]
    a32, s32, p32 = ref[torch.float32]
    assert len(a64.lr_path) == EPOCHS * NMB and a64.lr_path == a32.lr_path, "the two torch references took different learning-rate paths: the test is mis-built"
    assert s["lr"] == s64["learning_rate"] == s32["learning_rate"]
    ph, o = {}, 0
    for n, p in pol.named_parameters():
        ph[n] = s["p"][o:o + p.numel()].double().reshape(p.shape)
        o += p.numel()
    displacement = float(sum(a64.lr_path))  # Adam moves an entry by at most lr per step
    print(f"{'tensor':<18}{'q999 hip':>12}{'q999 torch32':>14}{'max hip':>12}{'max torch32':>13}")
    bad = []
    for n in p64:
        dh, d32 = (ph[n] - p64[n]).abs().flatten(), (p32[n] - p64[n]).abs().flatten()
        qh, q32 = torch.quantile(dh, 0.999).item(), torch.quantile(d32, 0.999).item()
        ulp = float(np.spacing(np.float32(p64[n].abs().max().item())))
        print(f"{n:<18}{qh:12.3e}{q32:14.3e}{dh.max().item():12.3e}{d32.max().item():13.3e}")
        if not qh <= max(8 * q32, ulp):
            bad.append((n, "q999", qh, q32))
        if not dh.max().item() <= displacement:
            bad.append((n, "max", dh.max().item(), displacement))
    assert not bad, bad
    for k in ("value_loss", "surrogate_loss", "entropy", "kl"):
        assert abs(s["stats"][k] - s64[k]) <= 8 * abs(s32[k] - s64[k]) + 1e-6 * abs(s64[k]), (k, s["stats"][k], s32[k], s64[k])


def test_symmetry_rides_along(case):
    from robot_lab_amd.symmetry import SymmetryTables

    pol, _, st32 = case
    rng = np.random.default_rng(11)

    def table(dim):
        perm = np.stack([np.arange(dim), rng.permutation(dim)]).astype(np.int32)
        return perm, np.concatenate([np.ones((1, dim)), rng.choice([-1.0, 1.0], size=(1, dim))]).astype(np.float32)

    kw = dict(symmetry=SymmetryTables(obs=table(OD), critic=table(CD), act=table(A)), mirror_loss=0.5)
    one, two = _update(pol, st32, **kw), _update(pol, st32, group=_Ranks(2), **kw)
    _same_state(two, one)
    assert two["stats"] == one["stats"] and two["norm"] == one["norm"] and one["stats"]["mirror_loss"] > 0 and one["stats"]["kl"] > 0


@pytest.mark.parametrize("lazy", [False, True])
def test_resume_is_exact(case, tmp_path, lazy):
    """lazy: the resumed learner is built without `max_rows_per_minibatch`, so its handle does not exist when the checkpoint is loaded - parameters
    and optimiser state wait in the Python layer and reach the device at the first update"""
    import torch

    pol, _, st32 = case
    gen = _gen(3)
    perms = [torch.randperm(B, device=DEV, generator=gen) for _ in range(3)]
    full = _hip(pol)
    for p in perms:
        stats = full.update(st32, perm=p)
    want = _snap(full, stats)
    full.close()
    first = _hip(pol)
    for p in perms[:2]:
        first.update(st32, perm=p)
    first.store_into(first.policy)
    torch.save(dict(model_state_dict=first.policy.state_dict(), optimizer_state_dict=first.optimizer_state_dict()), tmp_path / "model.pt")
    first.close()
    d = torch.load(tmp_path / "model.pt", map_location=DEV, weights_only=False)
    torch.manual_seed(9)
    from robot_lab_amd.ppo import ActorCritic

    resumed = _hip(ActorCritic(OD, CD, A, actor_hidden=HID, critic_hidden=HID), **({} if lazy else dict(max_rows_per_minibatch=MB)))  # other parameters
    assert (resumed.handle is None) == lazy
    resumed.policy.load_state_dict(d["model_state_dict"])
    resumed.load_from(resumed.policy)
    resumed.load_optimizer_state_dict(d["optimizer_state_dict"])
    if lazy:  # nothing reached a device yet; what was loaded is what a save before the first update would write
        assert resumed.handle is None and resumed.optimizer_state_dict() is d["optimizer_state_dict"]
        assert resumed.learning_rate == d["optimizer_state_dict"]["param_groups"][0]["lr"]
    else:
        assert _optimizer(resumed)[1] == 2 * EPOCHS * NMB
    got = _snap(resumed, resumed.update(st32, perm=perms[2]))
    resumed.close()
    _same_state(got, want)
    assert got["step"] == 3 * EPOCHS * NMB and got["stats"] == want["stats"]


def test_checkpoints_cross_learners(case):
    import torch

    from robot_lab_amd.ppo import PPO

    pol, _, st32 = case
    hip = _hip(pol)
    hip.update(st32, _gen())
    d = hip.optimizer_state_dict()
    m1, m2 = hip.flat("exp_avg"), hip.flat("exp_avg_sq")
    alg = PPO(copy.deepcopy(pol).to(DEV), **KW)
    alg.optimizer.load_state_dict(d)
    o = 0
    for p in alg.policy.parameters():
        st = alg.optimizer.state[p]
        assert torch.equal(st["exp_avg"].reshape(-1), m1[o:o + p.numel()]) and torch.equal(st["exp_avg_sq"].reshape(-1), m2[o:o + p.numel()])
        assert float(st["step"]) == EPOCHS * NMB
        o += p.numel()
    assert o == m1.numel() and alg.optimizer.param_groups[0]["lr"] == hip.learning_rate == _optimizer(hip)[0]
    hip.close()
    # the other way: what the torch learner's optimiser writes after an update of its own
    alg = PPO(copy.deepcopy(pol).to(DEV), **KW)
    alg.update(st32, _gen())
    hip = _hip(pol, max_rows_per_minibatch=MB)
    hip.load_optimizer_state_dict(copy.deepcopy(alg.optimizer.state_dict()))
    params = list(alg.policy.parameters())
    assert torch.equal(hip.flat("exp_avg"), torch.cat([alg.optimizer.state[p]["exp_avg"].reshape(-1) for p in params]))
    assert torch.equal(hip.flat("exp_avg_sq"), torch.cat([alg.optimizer.state[p]["exp_avg_sq"].reshape(-1) for p in params]))
    assert _optimizer(hip) == (alg.optimizer.param_groups[0]["lr"], EPOCHS * NMB) and hip.learning_rate == alg.optimizer.param_groups[0]["lr"]
    hip.close()


def test_a_failed_collective_closes_the_learner(case):
    """between rl_ppo_minibatch_local and rl_ppo_minibatch_apply the replicas depend on the collective: if it raises, the learner is closed (and
    says so) instead of staying half-way through a mini-batch"""
    from robot_lab_amd.capi import RlPpoError

    pol, _, st32 = case

    class Broken(_Ranks):
        def all_reduce_sum(self, t):
            if self.calls == 2:
                raise RuntimeError("link down")
            return super().all_reduce_sum(t)

    hip = _hip(pol, group=Broken(2))
    with pytest.raises(RlPpoError, match="CLOSED"):
        hip.update(st32, _gen())
    assert hip.handle is None and hip._wire is None


def test_set_world_and_the_split_are_refused_out_of_order(case):
    """the refusals of the C-ABI that need a live handle (tests/test_ppo_hip_world_abi.py has the rest)"""
    import torch

    pol, _, st32 = case
    hip = _hip(pol, max_rows_per_minibatch=MB)
    lib, h, err = hip.lib, hip.handle, lambda: hip.lib.rl_ppo_last_error().decode()
    for bad in (0, -2):
        assert lib.rl_ppo_set_world(h, bad) != 0 and "world_size" in err()
    assert lib.rl_ppo_minibatch_apply(h, hip._stream()) != 0 and "rl_ppo_minibatch_local" in err()
    assert lib.rl_ppo_set_flat(h, 0, C.c_void_p(hip.flat("exp_avg").data_ptr()), hip._stream()) != 0 and "2 or 3" in err()
    assert lib.rl_ppo_set_optimizer(h, 0.0, 1, hip._stream()) != 0 and "learning rate" in err()
    assert lib.rl_ppo_set_optimizer(h, 1e-3, -1, hip._stream()) != 0 and "step" in err()
    assert lib.rl_ppo_set_world(h, 2) == 0
    assert lib.rl_ppo_set_world(h, 2) != 0 and "already set" in err()
    hip.close()
    hip = _hip(pol, max_rows_per_minibatch=MB)
    hip.minibatch_grad(st32, torch.arange(MB, device=DEV))
    assert hip.lib.rl_ppo_set_world(hip.handle, 2) != 0 and "after the first mini-batch" in hip.lib.rl_ppo_last_error().decode()
    torch.cuda.synchronize()
    hip.close()
