"""Rollout storage, stochastic head and GAE (robot_lab_amd/csrc/rl_rollout.hip, csrc/rollout/rl_sample.h) on the GPU: exact families with
no tolerance (GAE through both record routes, constant advantages, the identity of the noise stream, slot discipline at the packing edges
of act_kernel) and bounds tied to an fp32 emulation's own distance from an fp64 reference (GAE, normalisation, log-probability, draws).
Helpers, case tables and the reasoning behind each family: tests/rollout_helpers.py; the teeth of both tiers: tests/test_rollout.py."""
import functools

import numpy as np
import pytest

import rollout_helpers as rh
from oracle.rollout import standard_normal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUTES = ("record_kernel", "deferred")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _storage(N, T, A, obs=3, critic=2, seed=0):
    from robot_lab_amd.rollout import RolloutStorage

    return RolloutStorage(N, T, obs, critic, A, seed=seed, device=DEV)


def _np(t):
    return t.cpu().numpy().copy()


def _act(st, mean=None, std=None, values=None):
    """one act with zero observations; mean 0 / std 1 by default.  Returns actions_out as numpy"""
    import torch

    N, A = st.num_envs, st.actions.shape[-1]
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    mean = z(N, A) if mean is None else _dev(mean)
    std = torch.ones(A, device=DEV) if std is None else _dev(std)
    values = z(N) if values is None else _dev(values)
    return _np(st.act(z(N, st.observations.shape[-1]), z(N, st.privileged_observations.shape[-1]), mean, std, values))


def _fill(st, c, route):
    """the case's T transitions through one record route: "record_kernel" = process_env_step with both flags; "deferred" = record_slots()
    closes the step with no launch and the test writes what rl_env_step_record with values == NULL writes: the raw reward, the byte 0 / 1 / 3"""
    import torch

    d8 = st.dones.view(torch.uint8)
    for t in range(st.num_transitions_per_env):
        _act(st, values=c["values"][t])
        if route == "record_kernel":
            st.process_env_step(_dev(c["rewards"][t]), _dev(c["terminated"][t]), _dev(c["time_outs"][t]), c["gamma"])
        else:
            st.record_slots()
            st.rewards[t] = _dev(c["rewards"][t])
            d8[t] = _dev(c["dones"][t])
    assert st.step == st.num_transitions_per_env


def _outputs(st):
    import torch

    torch.cuda.synchronize()
    return dict(returns=_np(st.returns), advantages=_np(st.advantages), rewards=_np(st.rewards), dones=_np(st.dones.view(torch.uint8)))


def _run_gae(c, route, normalize=False):
    """(outputs after the first compute_returns, after the second, the values the storage holds)"""
    T, N = c["values"].shape
    st = _storage(N, T, 2)
    _fill(st, c, route)
    st.compute_returns(_dev(c["last_values"]), c["gamma"], c["lam"], normalize_advantage=normalize)
    first = _outputs(st)
    st.compute_returns(_dev(c["last_values"]), c["gamma"], c["lam"], normalize_advantage=normalize)
    second = _outputs(st)
    values = _np(st.values)
    st.close()
    return first, second, values


# ---- exact tier: GAE families ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(rh.EXACT_CASES)), ids=[str(c) for c in rh.EXACT_CASES])
def test_gae_exact_families_on_both_record_routes(i):
    """nothing rounds in these cases (asserted in fp32 against fp64 by exact_gae_case), so returns, advantages, the bootstrapped rewards and
    the done bytes are the fp64 recursion's, bit for bit, through the record kernel and through the deferred route; after the deferred route
    every byte is 0 or 1; a second compute_returns changes nothing (no second bootstrap)."""
    c = rh.exact_case(i)
    want = c["want"]
    if c["time_outs"].size > 1 and rh.EXACT_CASES[i][6] > 0:
        assert (c["terminated"] & c["time_outs"]).any() and (c["dones"] == 1).any(), "the case holds envs that terminate and time out on one step"
    per_route = {}
    for route in ROUTES:
        first, second, values = _run_gae(c, route)
        rh.assert_bits_equal(values, c["values"], f"{route}: values")
        assert rh.exact_mismatches(first, want) == [], f"{route}: {rh.exact_mismatches(first, want)} differ from the fp64 recursion"
        for k in rh.EXACT_OUTPUTS:
            if k == "dones":
                assert set(np.unique(first[k])) <= {0, 1}
                np.testing.assert_array_equal(first[k], want[k], err_msg=route)
                np.testing.assert_array_equal(second[k], first[k], err_msg=f"{route}: second compute_returns")
            else:
                rh.assert_bits_equal(first[k], want[k], f"{route}: {k}")
                rh.assert_bits_equal(second[k], first[k], f"{route}: {k} after a second compute_returns")
        per_route[route] = first
    for k in rh.EXACT_OUTPUTS:
        np.testing.assert_array_equal(per_route["record_kernel"][k].view(np.uint8), per_route["deferred"][k].view(np.uint8), err_msg=k)


@pytest.mark.parametrize("T,N", [(24, 300), (1, 1), (1, 2)])
def test_constant_advantages_normalise_to_zero(T, N):
    """r = 1, V = 0, every step done: every raw advantage is 1, the mean is exactly 1 and the variance 0, so every normalised advantage is
    (1 - 1) * (1 / 1e-8) = +-0.0 and finite.  For N * T = 1 torch's unbiased std is NaN; norm_kernel divides by max(count - 1, 1) and gives 0."""
    c = dict(rewards=np.ones((T, N), dtype=np.float32), values=np.zeros((T, N), dtype=np.float32), last_values=np.full(N, 7.0, dtype=np.float32),
             dones=np.ones((T, N), dtype=np.uint8), terminated=np.ones((T, N), dtype=np.uint8), time_outs=np.zeros((T, N), dtype=np.uint8),
             gamma=0.99, lam=0.95)
    for route in ROUTES:
        raw, _, _ = _run_gae(c, route)
        rh.assert_bits_equal(raw["advantages"], np.ones((T, N)), f"{route}: raw advantages")
        first, second, _ = _run_gae(c, route, normalize=True)
        for out in (first, second):
            assert np.isfinite(out["advantages"]).all() and (out["advantages"] == 0.0).all(), route
            rh.assert_bits_equal(out["returns"], np.ones((T, N)), f"{route}: returns")


# ---- exact tier: the noise stream ------------------------------------------------------------------------------------------------------------
def _draws(N, A, steps, seed=5, T=None, obs=3, critic=2, std=None, skip=0):
    """z of `steps` consecutive acts (mean 0, std 1: the stored action is the draw itself) after `skip` recorded dummy transitions"""
    T = T or steps + skip
    st = _storage(N, T, A, obs, critic, seed)
    out = []
    for t in range(skip + steps):
        if st.step == T:
            st.clear()
        a = _act(st, std=std)
        slot = st.step
        st.record_slots()
        if t >= skip:
            rh.assert_bits_equal(_np(st.actions[slot]), a, "actions_out against the storage's actions (no clip)")
            out.append(a)
    st.close()
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _base_draws():
    return _draws(300, 29, 4)


def test_noise_stream_depends_on_env_column_counter_and_seed_only():
    z = _base_draws()
    assert np.isfinite(z).all() and len(np.unique(z)) > 0.99 * z.size
    rh.assert_bits_equal(_draws(37, 29, 4), z[:, :37], "z does not depend on N (37 against 300)")
    rh.assert_bits_equal(_draws(300, 5, 4), z[:, :, :5], "z does not depend on the action width (5 against 29)")
    rh.assert_bits_equal(_draws(300, 29, 4, obs=45, critic=7), z, "z does not depend on the observation widths")
    rh.assert_bits_equal(_draws(300, 29, 4, T=2), z, "z does not depend on T; clear() does not rewind the stream")
    rh.assert_bits_equal(_draws(300, 29, 1, skip=3)[0], z[3], "a fresh storage's fourth draw, after three recorded dummy transitions")
    other = _draws(300, 29, 1, seed=6)[0]
    assert not np.array_equal(other, z[0]) and (rh.bits(other) != rh.bits(z[0])).mean() > 0.99, "another seed gives other bits"
    for t in range(1, 4):
        assert (rh.bits(z[t]) != rh.bits(z[0])).mean() > 0.99, "another counter gives other bits"


@pytest.mark.parametrize("k", [-3, 2])
def test_power_of_two_std_scales_the_draw_bit_for_bit(k):
    z = _base_draws()
    a = _draws(300, 29, 4, std=np.full(29, 2.0 ** k, dtype=np.float32))
    rh.assert_bits_equal(a, z * np.float32(2.0 ** k), f"std = 2^{k}")


# ---- exact tier: slot discipline at the packing edges of act_kernel ---------------------------------------------------------------------------
PACKING = [(12, 85), (12, 86), (12, 170), (20, 52), (29, 33), (1024, 3)]


@pytest.mark.parametrize("A,N", PACKING, ids=[f"A{a}-N{n}" for a, n in PACKING])
def test_act_slots_at_the_packing_edges(A, N):
    """epb = 256 / ceil(A / 4) envs per workgroup: N = epb fills one exactly, epb + 1 puts one env in a second, 2 epb fills two; A = 1024 is one
    env per workgroup.  mu, sigma, values and both observation rows come back bit for bit, the draw is the stream's (that of the narrow
    storage), and slot t + 1 of every buffer is still all zero after the act of step t: nothing is written behind row N."""
    import torch

    assert rh.envs_per_block(12) == 85 and rh.envs_per_block(20) == 51 and rh.envs_per_block(29) == 32 and rh.envs_per_block(1024) == 1
    rng = np.random.default_rng(A * 1000 + N)
    T, od, cd = 3, 5, 7
    st = _storage(N, T, A, od, cd, seed=5)
    names = ("observations", "privileged_observations", "actions", "mu", "sigma", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages")
    for t in range(T - 1):
        f = dict(obs=rng.standard_normal((N, od)), critic=rng.standard_normal((N, cd)), mean=rng.standard_normal((N, A)), std=np.exp(rng.uniform(-1, 0.3, A)),
                 values=rng.standard_normal(N))
        f = {k: v.astype(np.float32) for k, v in f.items()}
        a = _np(st.act(_dev(f["obs"]), _dev(f["critic"]), _dev(f["mean"]), _dev(f["std"]), _dev(f["values"])))
        torch.cuda.synchronize()
        for name, want in (("observations", f["obs"]), ("privileged_observations", f["critic"]), ("mu", f["mean"]), ("sigma", np.broadcast_to(f["std"], (N, A))),
                           ("values", f["values"]), ("actions", a)):
            rh.assert_bits_equal(_np(getattr(st, name)[t]), want, f"step {t}: {name}")
        lp = _np(st.actions_log_prob[t])
        assert np.isfinite(lp).all() and (lp != 0).all()
        for name in names:
            assert not bool(getattr(st, name)[t + 1:].any()), f"step {t}: {name} written behind row N of slot {t}"
        st.record_slots()
    st.close()
    # the draws themselves: mean 0, std 1 against the 29-wide, 300-env storage's over the shared envs and columns
    z, n, w = _base_draws(), min(N, 300), min(A, 29)
    rh.assert_bits_equal(_draws(N, A, 1)[0][:n, :w], z[0][:n, :w], "the draw at a packing edge")


def test_act_dim_above_1024_is_refused():
    from robot_lab_amd.rollout import RlRolloutError

    with pytest.raises(RlRolloutError, match="1024"):
        _storage(3, 1, 1025)


# ---- bound tier -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("regime", rh.GAE_REGIMES)
def test_gae_within_the_fp32_emulations_error(regime, route):
    """max |kernel - fp64 recursion| <= K_GAE x max |fp32 recursion - fp64 recursion| on the bootstrapped rewards, returns and advantages, all three
    evaluated from the fp32 values the storage holds; "advantages = returns - values" holds in the kernel's own numbers, bit for bit (the
    running sum `a` stored in its place differs from it by one rounding and is no further from fp64, so only this identity sees it)."""
    c = rh.gae_regime(regime)
    emu, ref = rh.gae_refs(c)
    first, second, values = _run_gae(c, route)
    rh.assert_bits_equal(values, c["values"], "values")
    np.testing.assert_array_equal(first["dones"], ref["dones"])
    for k in rh.GAE_BOUND_OUTPUTS:
        if k == "rewards" and not c["time_outs"].any():
            rh.assert_bits_equal(first[k], c["rewards"], "rewards without a time out")
            continue
        rh.assert_bound(f"gae/{regime}/{route}", k, first[k], emu[k], ref[k], rh.K_GAE)
        rh.assert_bits_equal(second[k], first[k], f"{k} after a second compute_returns")
    rh.assert_bits_equal(first["advantages"], first["returns"] - values, "advantages = returns - values")


def _normalised(raw_case, route):
    first, _, _ = _run_gae(raw_case, route)
    second, third, _ = _run_gae(raw_case, route, normalize=True)
    rh.assert_bits_equal(third["advantages"], second["advantages"], "a second normalising compute_returns")
    return first["advantages"], second["advantages"]


@pytest.mark.parametrize("regime", ("production",) + rh.NORM_REGIMES)
def test_normalisation_within_the_fp32_emulations_error(regime):
    """the reference is the fp64 expression on the kernel's own raw fp32 advantages; the yardstick an fp32 numpy mean / unbiased std"""
    if regime == "production":
        c = rh.gae_regime("production")
    else:
        raw = rh.norm_regime(regime)
        T, N = raw.shape
        c = dict(rewards=raw, values=np.zeros((T, N), dtype=np.float32), last_values=np.zeros(N, dtype=np.float32), dones=np.ones((T, N), dtype=np.uint8),
                 terminated=np.ones((T, N), dtype=np.uint8), time_outs=np.zeros((T, N), dtype=np.uint8), gamma=0.99, lam=0.95)
    raw_k, got = _normalised(c, "record_kernel")
    if regime != "production":
        rh.assert_bits_equal(raw_k, c["rewards"], "the raw advantages of an all-done, zero-value storage are its rewards")
    rh.assert_bound(f"norm/{regime}", "advantages", got, rh.normalise_f32(raw_k), rh.normalise_f64(raw_k), rh.K_NORM)


@pytest.mark.parametrize("N", rh.LOGP_ENVS)
@pytest.mark.parametrize("A", rh.LOGP_WIDTHS)
def test_log_prob_within_the_fp32_emulations_error(A, N):
    """the reference is the fp64 Gaussian log-density at the stored fp32 actions, mu and sigma; the act-kernel route (the fused epilogue is
    bit-equal to it: tests/test_gpu_policy_exact.py)"""
    import torch

    st = _storage(N, len(rh.LOGP_REGIMES), A, seed=9)
    for t, regime in enumerate(rh.LOGP_REGIMES):
        mean, std = rh.logp_regime(regime, N, A, seed=A * 1000 + N)
        _act(st, mean=mean, std=std)
        st.record_slots()
        torch.cuda.synchronize()
        act, mu, sg, lp = (_np(getattr(st, n)[t]) for n in ("actions", "mu", "sigma", "actions_log_prob"))
        rh.assert_bits_equal(mu, mean, "mu")
        rh.assert_bits_equal(sg, np.broadcast_to(std, (N, A)), "sigma")
        rh.assert_bound(f"logp/{regime}/A{A}/N{N}", "log_prob", lp, rh.log_prob_f32(act, mu, sg), rh.log_prob_f64(act, mu, sg), rh.K_LOGP)
    st.close()


def test_draws_within_the_fp32_emulations_error():
    """z (mean 0, std 1) against oracle.rollout.standard_normal in fp64; the yardstick is Box-Muller in numpy fp32 on the same uniforms"""
    z = _draws(300, 29, 4, seed=1234)
    for counter in range(4):
        rh.assert_bound(f"draws/counter{counter}", "z", z[counter], rh.box_muller_f32(1234, 300, counter, 29), standard_normal(1234, 300, counter, 29), rh.K_DRAWS)
