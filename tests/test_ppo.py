"""The learner of robot_lab_amd/ppo.py (a restatement of rsl_rl's PPO.update; rsl-rl-lib itself is absent, so UNPINNED against the
library): its pieces against their definitions, on CPU.  The end-to-end check - a robot learns to follow velocity commands on this
simulator - is tests/test_gpu_train.py / tools/train_demo.py."""
import numpy as np
import pytest
import torch

from ppo_helpers import BRANCH_SHAPES, branch_case, branch_census, branch_classes, check_branches, fake_storage as _fake_storage, perturb, reference_gradients, tables
from robot_lab_amd.ppo import PPO, ActorCritic, gaussian_entropy, gaussian_kl, gaussian_log_prob


def test_gaussian_pieces_match_torch_distributions():
    g = torch.Generator().manual_seed(0)
    mu, mu2 = torch.randn(64, 12, generator=g), torch.randn(64, 12, generator=g)
    sd, sd2 = torch.rand(64, 12, generator=g) + 0.2, torch.rand(64, 12, generator=g) + 0.2
    a = torch.randn(64, 12, generator=g)
    p, q = torch.distributions.Normal(mu, sd), torch.distributions.Normal(mu2, sd2)
    torch.testing.assert_close(gaussian_log_prob(a, mu, sd), p.log_prob(a).sum(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gaussian_entropy(sd), p.entropy().sum(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gaussian_kl(mu, sd, mu2, sd2), torch.distributions.kl_divergence(p, q).sum(-1), rtol=1e-4, atol=1e-4)


def test_update_follows_the_advantage_and_adapts_the_learning_rate():
    torch.manual_seed(0)
    pol = ActorCritic(10, 14, 3, actor_hidden=(32, 32), critic_hidden=(32, 32))
    alg = PPO(pol, learning_rate=1e-3)
    st = _fake_storage(pol)
    with torch.no_grad():
        m0 = pol.actor(st.observations.reshape(-1, 10))[:, 0].mean().item()
        v0 = ((pol.critic(st.privileged_observations.reshape(-1, 14)).view(-1) - st.returns.view(-1)) ** 2).mean().item()
    out = alg.update(st, torch.Generator().manual_seed(1))
    with torch.no_grad():
        m1 = pol.actor(st.observations.reshape(-1, 10))[:, 0].mean().item()
        v1 = ((pol.critic(st.privileged_observations.reshape(-1, 14)).view(-1) - st.returns.view(-1)) ** 2).mean().item()
    assert m1 > m0, "the policy mean did not move along the advantage"
    assert v1 < v0, "the value loss did not go down"
    assert all(np.isfinite(v) for v in out.values()) and 1e-5 <= out["learning_rate"] <= 1e-2 and out["kl"] >= 0.0
    # gradient-norm clipping and the clipped surrogate keep a single update small: ratio stays near the clip range
    with torch.no_grad():
        mu, sd = pol.distribution(st.observations.reshape(-1, 10))
        ratio = torch.exp(gaussian_log_prob(st.actions.reshape(-1, 3), mu, sd) - st.actions_log_prob.view(-1))
    assert 0.5 < ratio.mean().item() < 1.5


# ---- the designed batch of tests/test_gpu_ppo_hip_branches.py: it is what it claims, and the parity bound on it has teeth (no GPU here) ----
WRONG_RULES = {"a": "no ratio clamp", "b": "the ratio clamp's gradient passed straight through (inr = 1)", "c": "min in place of max in the surrogate",
               "d": "unclipped value loss in place of the clipped one", "e": "the value clamp's gradient passed straight through (in2 = 1)",
               "f": "l1 / l2 selection swapped"}


def _loss_gradients(pol, st, wrong=None, clip=0.2, value_loss_coef=1.0, entropy_coef=0.01):
    """{parameter name: fp64 gradient} of `PPO.update`'s loss over the whole of `st` as one mini-batch, restated here so that ONE rule can be got
    wrong (`wrong`: a key of WRONG_RULES; None: the rule itself, checked against `PPO.update` below)"""
    import copy

    p = copy.deepcopy(pol).double()
    B = st.num_transitions_per_env * st.num_envs
    f = lambda t: t.reshape(B, -1).double()  # noqa: E731
    vo, ret, adv, lp_old = (f(x).view(-1) for x in (st.values, st.returns, st.advantages, st.actions_log_prob))
    mean, std = p.distribution(f(st.observations))
    ratio = torch.exp(gaussian_log_prob(f(st.actions), mean, std) - lp_old)
    value = p.critic(f(st.privileged_observations)).view(-1)
    clamped = ratio.clamp(1.0 - clip, 1.0 + clip)
    if wrong == "a":
        clamped = ratio
    elif wrong == "b":
        clamped = ratio + (clamped - ratio).detach()
    surrogate = (torch.min if wrong == "c" else torch.max)(-adv * ratio, -adv * clamped).mean()
    dv = value - vo
    dvc = dv.clamp(-clip, clip)
    if wrong == "e":
        dvc = dv + (dvc - dv).detach()
    l1, l2 = (value - ret) ** 2, (vo + dvc - ret) ** 2
    value_loss = (l1 if wrong == "d" else (torch.min if wrong == "f" else torch.max)(l1, l2)).mean()
    loss = surrogate + value_loss_coef * value_loss - entropy_coef * gaussian_entropy(std).mean()
    loss.backward()
    return {n: q.grad.detach() for n, q in p.named_parameters()}


def _bounds(ref):
    """{parameter name: (max|g64|, max(8 d, floor))}: the bound of ppo_helpers.compare_gradients, relative to the tensor's largest fp64 entry"""
    out = {}
    for n, g64 in ref[torch.float64].items():
        scale = g64.abs().max().item()
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        out[n] = (scale, max(8 * d, float(np.spacing(np.float32(scale))) / scale))
    return out


def _factors(pol, st, ref, wrong):
    """{parameter name: |gradient under the wrong rule - fp64 gradient| / (max|g64| x the tensor's bound)}"""
    g = _loss_gradients(pol, st, wrong)
    return {n: (g[n] - ref[torch.float64][n]).abs().max().item() / scale / bound for n, (scale, bound) in _bounds(ref).items()}


@pytest.mark.parametrize("shape", list(BRANCH_SHAPES))
def test_designed_batch_reaches_every_branch_with_margins(shape):
    """every outcome of the loss head holds >= 10 % of the rows, and no row is within 0.01 of a switch, by the fp64 forward alone"""
    pol, st, cls = branch_case(shape)
    census = check_branches(shape, cls)
    assert len(census) == 3 + 4 + 5 + 1 and bool(torch.isfinite(cls.r).all())
    assert all(bool(torch.isfinite(getattr(st, k)).all()) and getattr(st, k).dtype == torch.float32 for k in ("actions_log_prob", "advantages", "values", "returns", "mu", "sigma"))


def test_designed_batch_keeps_its_margins_under_the_symmetry_tables():
    """the 74 virtual rows of tests/test_gpu_ppo_hip_branches.py's symmetry case: a copy-1 row lands where the mirrored forward puts it, so its
    distance from the switches is a property of the batch's seed - checked here, in fp64"""
    pol, st, _ = branch_case("odd-37")
    c = branch_classes(pol, st, symmetry=tables(BRANCH_SHAPES["odd-37"]["dims"], 2))
    check_branches("odd-37 x 2 copies", c, share=None)
    assert c.rows == 74 and len(set(c.sur.tolist())) == 3 and len(set(c.val.tolist())) == 5


@pytest.mark.parametrize("shape", list(BRANCH_SHAPES))
def test_wrong_rules_show_on_the_designed_batch(shape):
    """each mistake the loss head could make moves the gradient of at least one parameter tensor by >= 100 x that tensor's parity bound
    max(8 d, floor) (d: the fp32 torch learner's distance from the fp64 one): the GPU test that passes has excluded all six"""
    pol, st, _ = branch_case(shape)
    ref, _ = reference_gradients(pol, st, device="cpu")
    for n, g in _loss_gradients(pol, st).items():  # the restated rule IS PPO.update's
        torch.testing.assert_close(g, ref[torch.float64][n], rtol=1e-9, atol=1e-12 * ref[torch.float64][n].abs().max().item())
    print(f"\n{shape}: sensitivity of the gradient bound on the designed batch")
    for wrong, what in WRONG_RULES.items():
        fac = _factors(pol, st, ref, wrong)
        n = max(fac, key=fac.get)
        print(f"  ({wrong}) {what:<66}{fac[n]:12.1f} x the bound of {n}")
        assert fac[n] >= 100, (wrong, what, fac)


def test_value_rules_do_not_show_on_the_old_batch():
    """why the designed batch exists: on the batch the other PPO tests share (fake_storage, T = 24, N = 256, parameters perturbed) no row's value
    is clipped, and the wrong value rules (d), (e), (f) stay below every tensor's bound"""
    torch.manual_seed(0)
    pol = ActorCritic(45, 235, 12)
    st = _fake_storage(pol, 24, 256, 45, 235, 12)
    perturb(pol)
    cls = branch_classes(pol, st)
    census = branch_census(cls)
    print(f"\nfake_storage 24 x 256: r {float(cls.r.min()):.3f} .. {float(cls.r.max()):.3f}, rows outside the band {int((cls.combo >= 0).sum())} of {cls.rows}, "
          f"max|dv| {float(cls.dv.abs().max()):.4f}, rows with a clipped value {int((cls.val != 0).sum())}")
    assert census["value in-band"] == 1.0 and census["surrogate tie"] > 0.99
    ref, _ = reference_gradients(pol, st, device="cpu")
    for wrong in "def":
        fac = _factors(pol, st, ref, wrong)
        n = max(fac, key=fac.get)
        print(f"  ({wrong}) {WRONG_RULES[wrong]:<66}{fac[n]:12.2e} x the bound of {n}")
        assert fac[n] < 1, (wrong, fac)


def test_state_dict_layout_is_rsl_rls():
    pol = ActorCritic(45, 235, 12)
    keys = set(pol.state_dict())
    assert {"std", "actor.0.weight", "actor.6.bias", "critic.0.weight", "critic.6.weight"} <= keys
    from robot_lab_amd.policy import MlpPolicy  # the inference side reads the same layout (from_state_dict)

    idx = sorted({int(k.split(".")[1]) for k in keys if k.startswith("actor.") and k.endswith(".weight")})
    assert idx == [0, 2, 4, 6] and hasattr(MlpPolicy, "from_state_dict") and hasattr(MlpPolicy, "set_weights")
