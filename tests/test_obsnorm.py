"""CPU tier of the observation normalisation: the RULE (`robot_lab_amd.ppo.EmpiricalNormalization`, torch) against its numpy restatement and
against the identity it implements, the checkpoint keys, and the teeth of the bound the GPU tier (tests/test_gpu_obsnorm.py) asserts for
csrc/rl_obsnorm.hip - all from tests/obsnorm_helpers.py."""
import numpy as np
import pytest
import torch

import obsnorm_helpers as oh
from robot_lab_amd.ppo import ActorCritic, EmpiricalNormalization

TODAYS_KEYS = ["std"] + [f"{net}.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4, 6) for p in ("weight", "bias")]


def _module_state(m):
    return dict(mean=m._mean.numpy().reshape(-1), var=m._var.numpy().reshape(-1), std=m._std.numpy().reshape(-1), count=int(m.count))


@pytest.mark.parametrize("dim,rows", [(1, (1, 5)), (3, (63, 64, 65)), (47, (257, 4, 300, 1))])
def test_the_torch_module_is_the_seven_lines(dim, rows):
    """fp64 module against the fp64 numpy restatement, update after update (the rate is ONE fp32 division in both)"""
    m = EmpiricalNormalization(dim).double()
    state = oh.fresh(dim)
    for u, x in enumerate(oh.bounded_batches(r, dim, 1, seed=10 * dim + r)[0] for r in rows):
        m.update(torch.from_numpy(x).double())
        state = oh.rule(state, x, np.float64)
        count = state["count"]
        got = _module_state(m)
        assert got["count"] == count
        for k in oh.VECTORS:
            np.testing.assert_allclose(got[k], state[k], rtol=1e-13, atol=1e-13, err_msg=f"{k} after update {u}")
    assert m._mean.shape == (1, dim) and m.count.dtype == torch.int64 and m.count.ndim == 0
    y = m(torch.from_numpy(x).double()).numpy()
    np.testing.assert_allclose(y, (x.astype(np.float64) - got["mean"]) / (got["std"] + 1e-2), rtol=1e-14, atol=0)  # forward, on the module's own state


def test_the_state_is_the_statistics_of_the_concatenation():
    """the identity the rule implements: after B1 .. Bk, mean / var are the population mean / variance of all rows seen.  fp64, equal batches
    (the rate n / count is then 1 / k: an fp32 number for k = 1, 2, 4 and rounded once for k = 3, which the 1e-12 below does not forgive - so
    the identity is checked after 1, 2 and 4 batches) and unequal ones with power-of-two counts"""
    rng = np.random.default_rng(3)
    for sizes in ((64, 64, 128, 256), (32, 32, 64), (512,)):
        m = EmpiricalNormalization(7).double()
        seen = []
        for n in sizes:
            x = 5.0 + 3.0 * rng.standard_normal((n, 7))
            seen.append(x)
            m.update(torch.from_numpy(x))
            allx = np.concatenate(seen)
            got = _module_state(m)
            assert got["count"] == len(allx)
            for k, want in (("mean", allx.mean(0)), ("var", allx.var(0)), ("std", allx.std(0))):
                err = np.abs(got[k] - want).max() / max(1.0, np.abs(want).max())
                assert err <= 1e-12, (sizes, n, k, err)


def test_an_eval_module_does_not_move():
    m = EmpiricalNormalization(5)
    m.update(torch.randn(16, 5))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.eval()
    m.update(100.0 + torch.randn(16, 5))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    m.train()
    m.update(100.0 + torch.randn(16, 5))
    assert int(m.count) == 32 and not torch.equal(m._mean, before["_mean"])


@pytest.mark.parametrize("actor_on,critic_on", [(False, False), (True, False), (False, True), (True, True)])
def test_state_dict_keys_and_shapes(actor_on, critic_on):
    pol = ActorCritic(45, 235, 12, actor_obs_normalization=actor_on, critic_obs_normalization=critic_on)
    sd = pol.state_dict()
    want = list(TODAYS_KEYS)
    for name, on, dim in (("actor_obs_normalizer", actor_on, 45), ("critic_obs_normalizer", critic_on, 235)):
        assert isinstance(getattr(pol, name), EmpiricalNormalization if on else torch.nn.Identity)
        if on:
            want += [f"{name}._mean", f"{name}._var", f"{name}._std", f"{name}.count"]
            assert sd[f"{name}._mean"].shape == sd[f"{name}._var"].shape == sd[f"{name}._std"].shape == (1, dim)
            assert sd[f"{name}.count"].shape == () and sd[f"{name}.count"].dtype == torch.int64
            assert float(sd[f"{name}._mean"].abs().max()) == 0 and bool((sd[f"{name}._var"] == 1).all()) and bool((sd[f"{name}._std"] == 1).all())
    assert sorted(sd) == sorted(want)
    assert [n for n, _ in pol.named_parameters()] == [n for n, _ in ActorCritic(45, 235, 12).named_parameters()]  # the flat layouts do not change


def test_flags_off_is_todays_module_and_loads_todays_checkpoints():
    torch.manual_seed(0)
    old = ActorCritic(10, 14, 3)
    assert sorted(old.state_dict()) == sorted(TODAYS_KEYS)
    new = ActorCritic(10, 14, 3, actor_obs_normalization=False, critic_obs_normalization=False)
    new.load_state_dict(old.state_dict())
    x = torch.randn(4, 10)
    assert torch.equal(new.distribution(x)[0], old.actor(x))
    with pytest.raises(RuntimeError, match="actor_obs_normalizer"):  # a key mismatch raises, as load_state_dict does
        ActorCritic(10, 14, 3, actor_obs_normalization=True).load_state_dict(old.state_dict())
    with pytest.raises(RuntimeError, match="critic_obs_normalizer"):
        old.load_state_dict(ActorCritic(10, 14, 3, critic_obs_normalization=True).state_dict())


def test_the_update_rule_sees_the_normaliser():
    """PPO.update evaluates actor(actor_obs_normalizer(obs)) / critic(critic_obs_normalizer(obs)): with statistics far from (0, 1) the losses
    differ from those of the same networks without the modules"""
    torch.manual_seed(1)
    pol = ActorCritic(6, 8, 2, actor_hidden=(16,), critic_hidden=(16,), actor_obs_normalization=True, critic_obs_normalization=True)
    pol.actor_obs_normalizer.update(3.0 + 2.0 * torch.randn(64, 6))
    pol.critic_obs_normalizer.update(-1.0 + 0.5 * torch.randn(64, 8))
    x, c = torch.randn(5, 6), torch.randn(5, 8)
    assert torch.equal(pol.distribution(x)[0], pol.actor((x - pol.actor_obs_normalizer._mean) / (pol.actor_obs_normalizer._std + 1e-2)))
    assert torch.equal(pol.evaluate(c), pol.critic((c - pol.critic_obs_normalizer._mean) / (pol.critic_obs_normalizer._std + 1e-2)))
    assert not torch.equal(pol.distribution(x)[0], pol.actor(x))
    assert torch.equal(pol.distribution(x, normalized=True)[0], pol.actor(x))


# ---- the bound's teeth ----------------------------------------------------------------------------------------------------------------------
TEETH_SHAPES = [(257, 1), (4096, 1)]  # more than one tile (the cross term needs two); one column: the vector IS the offset column


def _errors(batches, stats):
    ref = oh.replay(batches, np.float64)
    with np.errstate(invalid="ignore"):
        got = oh.replay(batches, oh.F, stats)
    return {k: np.abs(got[k].astype(np.float64) - ref[k]) for k in oh.VECTORS}


@pytest.mark.parametrize("n_rows,dim", TEETH_SHAPES)
def test_the_bound_rejects_a_cancelling_variance_and_a_merge_without_cross_term(n_rows, dim):
    """On the offset column (mean 1e3, std 1e-2) of the bounded family both defects leave the bound K_CAP x (fp32 numpy rule's distance from
    the fp64 rule).  Measured here (three updates, seed 1): the cancelling variance misses var by 2.1e-2 at 257 rows and 9.8e-5 at 4096, where
    the yardstick is 1.3e-8 and 7.5e-9 (1.6e6 x and 1.3e4 x); the merge of 64-row tiles without delta^2 by 1.8e-6 and 1.4e-6 (138 x and 193 x)."""
    batches = oh.bounded_batches(n_rows, dim, 3, seed=1)
    yard = {k: v.max() for k, v in _errors(batches, oh.two_pass).items()}
    assert yard["var"] > 0
    for name, stats in (("sum x^2 / n - mean^2", oh.naive_variance), ("no cross term", lambda x, dt: oh.tiles(x, dt, cross_term=False))):
        err = _errors(batches, stats)["var"]
        worst = np.nanmax(err[list(oh.OFFSET_COLUMNS)]) if not np.isnan(err[list(oh.OFFSET_COLUMNS)]).all() else np.inf
        print(f"[obsnorm-teeth] {n_rows}x{dim} {name}: var error {worst:.3e} on the offset column, yardstick {yard['var']:.3e}, ratio {worst / yard['var']:.1f}")
        assert worst > oh.K_CAP * yard["var"], (name, worst, yard["var"])


@pytest.mark.parametrize("n_rows,dim", TEETH_SHAPES + [(65, 47), (63, 3)])
def test_the_fp32_two_pass_tiles_pass(n_rows, dim):
    """what a kernel that kept everything in fp32 - two passes inside a tile, Chan's merge in tile order - would give: inside the bound at its
    cap, so the bound asks for the formulation and not for fp64"""
    batches = oh.bounded_batches(n_rows, dim, 3, seed=1)
    yard, err = _errors(batches, oh.two_pass), _errors(batches, oh.tiles)
    for k in oh.VECTORS:
        assert err[k].max() <= oh.K_CAP * yard[k].max(), (k, err[k].max(), yard[k].max())


def test_the_exact_family_is_not_empty():
    n = 0
    for rows in oh.EXACT_ROWS:
        for dim in oh.DIMS:
            for updates in (1, 2):
                start, batches, states = oh.exact_batches(rows, dim, updates, seed=rows + dim + updates)
                assert len(batches) == updates and states[-1]["count"] == rows * updates
                if rows != 64:  # (256 rows: an fp32 running sum of (x - mean)^2 needs 30 bits; the kernel's tile sums are fp64)
                    n += 1
                    continue
                # 64 rows: the fp32 rule on numpy's own fp32 statistics lands on the same bits - nothing rounds in any order
                s32 = dict(mean=start["mean"].astype(oh.F), var=start["var"].astype(oh.F), std=start["std"].astype(oh.F), count=0)
                got = oh.replay(batches, oh.F, oh.two_pass, s32)
                for k in oh.VECTORS:
                    oh.assert_bits_equal(got[k], states[-1][k].astype(oh.F), f"{rows}x{dim}, {updates} updates, {k}")
                n += 1
    assert n == 24
