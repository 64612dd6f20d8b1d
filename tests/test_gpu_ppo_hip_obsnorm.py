"""`-m gpu`: observation normalisation inside the HIP PPO learner (`rl_ppo_set_obs_normalization`, the NORM instantiations of
ppo_gemm_kernel in csrc/rl_ppo.hip, `ppo_hip.HipPPO(obs_normalizers=...)`), alone and together with symmetry.

Setup: tests/obsnorm_symmetry_helpers.py (asymmetric statistics from `EmpiricalNormalization.update`, one constant column per group, raw rows of
the same column distributions, random signed-permutation tables).  Comparators, never the code under test:
  exact     a `HipPPO` WITHOUT the call on rows that were normalised before by `ObsNormalizer.apply` (rl_obsnorm_apply) - with symmetry: on the
            materialised rows, mirrored by torch (a gather and a sign flip: exact) and then normalised by `ObsNormalizer.apply` - bit for bit
  bounded   the torch rule `ppo.PPO(symmetry=...)` on the raw rows in fp64 (pinned to mirror-then-normalise by tests/test_ppo_obsnorm_symmetry.py);
            the same in fp32 measures what fp32 round-off alone does (d).  Bounds: those of tests/test_gpu_ppo_hip_symmetry.py, unchanged -
            e <= max(8 d, one fp32 spacing) per tensor; q999 <= max(8 q999_32, ulp); max <= the sum of the learning rates; one learning-rate path
The e / d tables are profiles/ppo_hip_obsnorm_parity.txt."""
import copy
import ctypes as C
import types

import numpy as np
import pytest

import obsnorm_symmetry_helpers as H
from ppo_helpers import DEV, cast as _cast, compare_gradients, gen as _gen, perm as perm_of, split as _split, tables, torch_learner as _torch_learner

pytestmark = pytest.mark.gpu

B, MB = H.B, H.MB
STATE = ("parameters", "exp_avg", "exp_avg_sq")


def _idx(rows):
    return perm_of(B)[:rows]


def _hip(pol, **kw):
    from robot_lab_amd.ppo_hip import HipPPO

    return HipPPO(copy.deepcopy(pol).to(DEV), **kw)


def _applied(st32, hs):
    """`st32` with both observation matrices through `ObsNormalizer.apply` (a group without a handle keeps its raw rows)"""
    out = copy.copy(st32)
    for k, h in zip(("observations", "privileged_observations"), hs):
        if h is not None:
            x = getattr(st32, k)
            setattr(out, k, h.apply(x.reshape(-1, x.shape[-1]).contiguous()).reshape(x.shape))
    return out


def _materialised(st32, tab, idx, hs):
    """the n_sym len(idx) network-input rows as a 1 x rows storage: mirrored by torch (exact), then `ObsNormalizer.apply` (no handle: raw)"""
    import torch

    rows = lambda t: t.reshape(B, -1)[idx]  # noqa: E731
    out = types.SimpleNamespace(num_transitions_per_env=1, num_envs=tab.n_sym * len(idx))
    for k, table, h in (("observations", tab.obs, hs[0]), ("privileged_observations", tab.critic, hs[1]), ("actions", tab.act, None)):
        x = H.mirrored(rows(getattr(st32, k)), table, tab.n_sym).contiguous()
        setattr(out, k, x if h is None else h.apply(x))
    for k in ("values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
        setattr(out, k, rows(getattr(st32, k)).repeat(tab.n_sym, 1))
    for k, v in list(vars(out).items()):
        if torch.is_tensor(v):
            setattr(out, k, v.unsqueeze(0).contiguous())
    return out


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, tuple) else (t,)):
            if x is not None:
                x.close()


# ---- 1. exact, no symmetry ---------------------------------------------------------------------------------------------------------
SMALL = dict(hidden=(32,))
EXACT = {"a1-1000": (dict(), 1000), "a1-37": (dict(), 37), "a1-1536": (dict(), MB),
         "1x17-37": (dict(dims=(1, 17, 3), **SMALL), 37), "512x512-1000": (dict(dims=(512, 512, 3), **SMALL), 1000),
         "45x235-small-1000": (dict(dims=(45, 235, 12), **SMALL), 1000),
         "actor-only-1000": (dict(critic=False, **SMALL), 1000), "critic-only-37": (dict(actor=False, **SMALL), 37)}


@pytest.mark.parametrize("name", list(EXACT))
def test_fused_normalisation_is_rl_obsnorm_apply_bit_for_bit(name):
    """`HipPPO(obs_normalizers=...)` on raw rows == `HipPPO` on rows pre-normalised by `ObsNormalizer.apply`: the gradient of one mini-batch, and after
    one whole update the parameters, both Adam moments and the returned statistics - every bit.  1000 rows: no multiple of a tile or a slice;
    37: one partial tile; 1536: the whole first mini-batch; widths 1 / 17 (one partial slice), 45 / 235, 512 / 512 (the widest input: 32 whole
    slices, four column tiles of the dW problem); one group normalised, each way round (the other passes through the same launch)."""
    import torch

    case_kw, rows = EXACT[name]
    pol, st = H.case(**case_kw)
    st32, hs, idx = _cast(st, torch.float32), H.handles(pol), _idx(rows)
    fused, plain = _hip(pol, max_rows_per_minibatch=MB, obs_normalizers=hs), _hip(pol, max_rows_per_minibatch=MB)
    assert f"obs_normalizers={[n for n, h in zip(('actor', 'critic'), hs) if h is not None]}" in repr(fused) and "obs_normalizers" not in repr(plain)
    pre = _applied(st32, hs)
    g_fused, g_plain = fused.minibatch_grad(st32, idx), plain.minibatch_grad(pre, idx)
    assert bool(torch.isfinite(g_plain).all()) and float(g_plain.abs().max()) > 0
    assert torch.equal(g_fused, g_plain), f"{int((g_fused != g_plain).sum())} of {g_plain.numel()} gradient words differ"
    s_fused, s_plain = fused.update(st32, _gen()), plain.update(pre, _gen())
    assert s_fused == s_plain, (s_fused, s_plain)
    for w in STATE:
        assert torch.equal(fused.flat(w), plain.flat(w)), w
    _close(fused, plain, hs)


# ---- 2. exact, with symmetry -------------------------------------------------------------------------------------------------------
SYM_CASES = [(1000, 4, True), (37, 2, True), (MB, 2, False)]
SYM_IDS = ["1000x4", "37x2", "1536x2-critic-replicated"]


def _sym_pair(pol, st32, tab, idx, hs, normalised):
    """(gradient of HipPPO(symmetry=tab[, obs_normalizers]) on the raw rows, gradient of a plain HipPPO on the materialised rows); both fixed schedule"""
    import torch

    sym = _hip(pol, max_rows_per_minibatch=MB, symmetry=tab, schedule="fixed", **(dict(obs_normalizers=hs) if normalised else {}))
    plain = _hip(H.without_normalizers(pol), max_rows_per_minibatch=tab.n_sym * MB, schedule="fixed")  # (the dW chunk split follows the allocation)
    mat = _materialised(st32, tab, idx, hs if normalised else (None, None))
    g_sym = sym.minibatch_grad(st32, idx)
    g_mat = plain.minibatch_grad(mat, torch.arange(tab.n_sym * len(idx), device=DEV))
    _close(sym, plain)
    return g_sym, g_mat


@pytest.mark.parametrize("rows,n_sym,critic", SYM_CASES, ids=SYM_IDS)
def test_precondition_mirror_in_the_fetch_equals_materialised_rows(rows, n_sym, critic):
    """Normalisation OFF on both sides (no new code): the SYM fetch on raw rows == the plain learner on the rows written out, bit for bit.  What
    the exact claim of the next test stands on."""
    import torch

    pol, st = H.case()
    bare = H.without_normalizers(pol)
    g_sym, g_mat = _sym_pair(bare, _cast(st, torch.float32), tables((H.OD, H.CD, H.A), n_sym, critic), _idx(rows), (None, None), False)
    assert bool(torch.isfinite(g_mat).all()) and float(g_mat.abs().max()) > 0
    assert torch.equal(g_sym, g_mat), f"{int((g_sym != g_mat).sum())} of {g_mat.numel()} gradient words differ"


@pytest.mark.parametrize("rows,n_sym,critic", SYM_CASES, ids=SYM_IDS)
def test_mirror_then_normalise_in_the_fetch_is_exact(rows, n_sym, critic):
    """`HipPPO(symmetry=tab, obs_normalizers=...)` on raw rows == a plain `HipPPO` on the materialised mirrored-then-normalised rows, bit for bit:
    the fetch normalises behind the mirror with the statistics of the destination column.  Copy boundaries inside a tile, a slice and a dW
    chunk (1000 x 4), at an odd row of one partial tile (37 x 2), the whole mini-batch with the critic's rows replicated (1536 x 2)."""
    import torch

    pol, st = H.case()
    hs = H.handles(pol)
    g_sym, g_mat = _sym_pair(pol, _cast(st, torch.float32), tables((H.OD, H.CD, H.A), n_sym, critic), _idx(rows), hs, True)
    assert bool(torch.isfinite(g_mat).all()) and float(g_mat.abs().max()) > 0
    assert torch.equal(g_sym, g_mat), f"{int((g_sym != g_mat).sum())} of {g_mat.numel()} gradient words differ"
    _close(hs)


# ---- 3. bounded by the fp32 reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.CASES))
def test_gradient_parity_with_symmetry_and_normalisation(name):
    """e <= max(8 d, one fp32 spacing of max|g64| relative to it) per parameter tensor, against the torch rule on the RAW rows in fp64"""
    import torch

    pol, st = H.case()
    tab, idx, kw = H._tables(2), _idx(1000), H.CASES[name]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        alg = _torch_learner(pol, dtype, symmetry=tab, num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30, **kw)
        alg.update(_cast(st, dtype, rows=idx), _gen(5))
        ref[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}
    hs = H.handles(pol)
    hip = _hip(pol, max_rows_per_minibatch=MB, symmetry=tab, obs_normalizers=hs, **kw)
    g_hip = _split(hip.minibatch_grad(_cast(st, torch.float32), idx), pol)
    torch.cuda.synchronize()
    bad = compare_gradients(f"{name}: 1000 rows x 2 copies, both groups normalised in the fetch", g_hip, ref)
    assert not bad, f"gradient error above 8 x the fp32 torch learner's: {bad}"
    _close(hip, hs)


@pytest.mark.parametrize("name", list(H.CASES))
def test_one_update_with_symmetry_and_normalisation_matches_the_torch_rule(name):
    import torch

    pol, st = H.case()
    tab, kw = H._tables(2), dict(H.CASES[name], desired_kl=H.DESIRED_KL)  # (a path that rises, holds and falls: obsnorm_symmetry_helpers.py)
    a64, a32 = _torch_learner(pol, torch.float64, symmetry=tab, **kw), _torch_learner(pol, torch.float32, symmetry=tab, **kw)
    s64, s32 = a64.update(_cast(st, torch.float64), _gen(H.UPDATE_SEED)), a32.update(_cast(st, torch.float32), _gen(H.UPDATE_SEED))
    assert len(a64.lr_path) == 20 and a64.lr_path == a32.lr_path, "the two torch references took different learning-rate paths: the inputs are mis-chosen"
    hs = H.handles(pol)
    hip = _hip(pol, symmetry=tab, obs_normalizers=hs, **kw)
    s_hip = hip.update(_cast(st, torch.float32), _gen(H.UPDATE_SEED))
    out = hip.store_into(copy.deepcopy(pol).to(DEV))
    torch.cuda.synchronize()
    p64 = {n: p.detach().double().cpu() for n, p in a64.policy.named_parameters()}
    p32 = {n: p.detach().double().cpu() for n, p in a32.policy.named_parameters()}
    ph = {n: p.detach().double().cpu() for n, p in out.named_parameters()}
    displacement = float(sum(a64.lr_path))  # Adam moves an entry by at most lr per step
    print(f"\n{name}: one update (5 epochs x 4 mini-batches of 1536 rows x 2 copies)\n{'tensor':<18}{'q999 hip':>12}{'q999 torch32':>14}{'max hip':>12}{'max torch32':>13}")
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
    print({k: (s_hip[k], s32[k], s64[k]) for k in s64})
    for k in [k for k in s64 if k != "learning_rate"]:
        assert abs(s_hip[k] - s64[k]) <= 8 * abs(s32[k] - s64[k]) + 1e-6 * abs(s64[k]), (k, s_hip[k], s32[k], s64[k])
    assert s_hip["learning_rate"] == s64["learning_rate"] == s32["learning_rate"]
    _close(hip, hs)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_update_is_deterministic():
    import torch

    pol, st = H.case()
    st32, tab, runs = _cast(st, torch.float32), H._tables(3), []
    for _ in range(2):
        hs = H.handles(pol)
        hip = _hip(pol, symmetry=tab, obs_normalizers=hs, mirror_loss=0.5)
        hip.update(st32, _gen())
        runs.append([hip.flat(w).cpu() for w in STATE])
        _close(hip, hs)
    for x, y in zip(*runs):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


# ---- 5. the statistics are read when the kernels run ---------------------------------------------------------------------------------
def test_statistics_are_read_at_launch_time():
    """an `ObsNormalizer.update` enqueued between two `minibatch_grad` calls changes the second gradient, and by exactly what a fresh learner built
    on the new statistics computes: the handle keeps pointers, not a copy"""
    import torch

    pol, st = H.case()
    st32, tab, idx = _cast(st, torch.float32), H._tables(2), _idx(1000)
    hs = H.handles(pol)
    hip = _hip(pol, max_rows_per_minibatch=MB, symmetry=tab, obs_normalizers=hs)
    g0 = hip.minibatch_grad(st32, idx)
    assert torch.equal(hip.minibatch_grad(st32, idx), g0)
    hs[0].update((3.0 * st32.observations.reshape(B, -1)[:512] + 1.0).contiguous())
    hs[1].update((0.5 * st32.privileged_observations.reshape(B, -1)[:512] - 2.0).contiguous())
    g1 = hip.minibatch_grad(st32, idx)
    assert not torch.equal(g1, g0) and bool(torch.isfinite(g1).all())
    fresh_hs = []
    for h in hs:  # new handles that START on the new statistics
        from robot_lab_amd.obsnorm import ObsNormalizer

        f = ObsNormalizer(h.dim, h.eps, max_rows=4096, device=DEV)
        f.set_state(*h.get_state())
        fresh_hs.append(f)
    fresh = _hip(pol, max_rows_per_minibatch=MB, symmetry=tab, obs_normalizers=tuple(fresh_hs))
    assert torch.equal(fresh.minibatch_grad(st32, idx), g1)
    _close(hip, fresh, hs, tuple(fresh_hs))


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    import torch

    from robot_lab_amd.obsnorm import ObsNormalizer, load_obsnorm_library
    from robot_lab_amd.ppo_hip import HipPPO, RlPpoError

    pol, st = H.case()
    st32, idx, hs = _cast(st, torch.float32), _idx(37), H.handles(pol)
    launches = load_obsnorm_library().rl_obsnorm_launch_count
    before = launches()
    # -- the library (include/rl_ppo.h): every refusal comes with a reason and leaves the handle a learner without the call
    hip = _hip(H.without_normalizers(pol), max_rows_per_minibatch=64)
    lib, err = hip.lib, lambda: (hip.lib.rl_ppo_last_error() or b"").decode()  # noqa: E731
    (am, asd, ae), (cm, csd, ce) = (h.device_pointers() for h in hs)
    call = lambda *a: lib.rl_ppo_set_obs_normalization(*[x if isinstance(x, float) else C.c_void_p(x) for x in a])  # noqa: E731
    for args, reason in (((None, am, asd, ae, cm, csd, ce), "null argument"),
                         ((hip.handle.value, None, None, 0.0, None, None, 0.0), "both groups are null"),
                         ((hip.handle.value, am, None, ae, cm, csd, ce), "actor mean and std are both given or both null"),
                         ((hip.handle.value, am, asd, ae, None, csd, ce), "critic mean and std are both given or both null"),
                         ((hip.handle.value, am, asd, -1e-3, cm, csd, ce), "actor eps must be finite and >= 0"),
                         ((hip.handle.value, am, asd, ae, cm, csd, float("nan")), "critic eps must be finite and >= 0"),
                         ((hip.handle.value, am, asd, ae, cm, csd, float("inf")), "critic eps must be finite and >= 0")):
        assert call(*args) != 0 and reason in err(), (args, err())
    reference = _hip(H.without_normalizers(pol), max_rows_per_minibatch=64)
    g = hip.minibatch_grad(st32, idx)
    assert torch.equal(g, reference.minibatch_grad(st32, idx)), "a refused call changed the learner"
    assert call(hip.handle.value, am, asd, ae, cm, csd, ce) != 0 and "refused after the first rl_ppo_minibatch_grad / rl_ppo_update" in err()
    assert torch.equal(hip.minibatch_grad(st32, idx), g)
    _close(hip, reference)
    hip = _hip(pol, max_rows_per_minibatch=64, obs_normalizers=hs)
    assert call(hip.handle.value, am, asd, ae, cm, csd, ce) != 0 and "already set" in err()
    with pytest.raises(RlPpoError, match="already set"):
        hip._set_obs_normalization(hs)
    hip.close()
    # -- the class (ppo_hip.HipPPO): a ValueError that says why, before a handle exists
    narrow = ObsNormalizer(H.OD - 1, 1e-2, max_rows=64, device=DEV)
    with pytest.raises(ValueError, match="the actor's normaliser is 44 columns wide, the network's input 45"):
        _hip(pol, obs_normalizers=(narrow, hs[1]))
    with pytest.raises(ValueError, match="the critic's normaliser is 45 columns wide, the network's input 235"):
        _hip(pol, obs_normalizers=(hs[0], hs[0]))
    with pytest.raises(ValueError, match="actor_obs_normalizer is nn.Identity"):
        _hip(H.without_normalizers(pol), obs_normalizers=hs)
    with pytest.raises(ValueError, match="no handle for the critic, but the policy's critic_obs_normalizer is a EmpiricalNormalization"):
        _hip(pol, obs_normalizers=(hs[0], None))
    unindexed = ObsNormalizer(H.OD, 1e-2, max_rows=64, device="cuda")  # the same device as cuda:0: accepted
    _hip(pol, max_rows_per_minibatch=64, obs_normalizers=(unindexed, hs[1])).close()
    unindexed.close()
    with pytest.raises(ValueError, match="at least one handle"):
        _hip(pol, obs_normalizers=(None, None))
    if torch.cuda.device_count() > 1:
        other = ObsNormalizer(H.OD, 1e-2, max_rows=64, device="cuda:1")
        with pytest.raises(ValueError, match="lives on cuda:1"):
            _hip(pol, obs_normalizers=(other, hs[1]))
        other.close()
    else:  # one device: the check is exercised on a stand-in that says it lives elsewhere
        elsewhere = types.SimpleNamespace(dim=H.OD, device=torch.device("cuda:1"), eps=1e-2)
        with pytest.raises(ValueError, match="lives on cuda:1"):
            HipPPO(copy.deepcopy(pol).to(DEV), obs_normalizers=(elsewhere, hs[1]))
    assert launches() == before, "a refusal launched a normalisation kernel"
    _close(narrow, hs)
