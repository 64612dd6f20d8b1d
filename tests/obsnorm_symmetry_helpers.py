"""The one copy of what the tests of observation normalisation TOGETHER WITH symmetry share (tests/test_ppo_obsnorm_symmetry.py on the CPU,
tests/test_gpu_ppo_hip_obsnorm.py on the GPU).  Reuses tests/ppo_helpers.py and tests/obsnorm_helpers.py, changes neither.

  policy      ActorCritic(45, 235, 12) with BOTH normalisers on, parameters perturbed after the storage was drawn (`PERTURB_SEED`)
  statistics  made legitimately and asymmetrically: `EmpiricalNormalization.update` is fed four batches whose column c is drawn around a mean in
              [-3, 3] with a spread log-uniform in [0.05, 20]; one column of each group is held CONSTANT (std = 0: the divisor is eps alone)
  storage     `fake_storage`'s recipe at T = 24, N = 256 with the RAW observations drawn from the same column distributions, so the normalised
              (unmirrored) inputs are O(1); values through the critic's normaliser
  tables      random signed permutations from `ppo_helpers.tables`: a mirrored column meets the statistics of ANOTHER column, which is the point
  the rule    `materialise(st, tab, idx, pol)`: mirror the raw rows, THEN normalise with the statistics of the destination column - the rows the
              unchanged plain learner is given on an identity-normaliser copy of the policy (`without_normalizers`)
`torch` is imported inside the functions: the module imports wherever its users do."""
import copy
import functools
import types

import numpy as np

from obsnorm_helpers import EPS
from ppo_helpers import DEV, tables

T, N, OD, CD, A = 24, 256, 45, 235, 12
B, MB = T * N, T * N // 4
CONSTANT = {"actor": (5, 1.5), "critic": (17, -2.25)}  # (column, its value) held constant: exactly representable, so its mean is exact and its var 0
# (a group narrower than that holds its last column; a group of ONE column holds none - it would have nothing else)
STAT_SEED, STAT_BATCHES, STAT_ROWS = 21, 4, 512
# With these seeds the fp64 and the fp32 torch learner walk the same 20-step learning-rate path on the inputs below, for every case of
# CASES (asserted by tests/test_ppo_obsnorm_symmetry.py on the CPU and again by the GPU tests that rely on it)
PERTURB_SEED, UPDATE_SEED = 1, 1
# The KL target of the whole-update tests.  With the default 0.01 the KL of these inputs (0.02 - 0.14) only ever lowers the learning rate, to its
# floor: a path that hardly depends on the statistic.  With 0.1 the fp64 torch rule's path rises (KL < 0.05), HOLDS (0.05 .. 0.2: either
# threshold is near) and falls in every case of CASES, so an error in the KL statistic of a learner shows as another path.
DESIRED_KL = 0.1
CASES = {"augmentation": dict(), "mirror-loss": dict(mirror_loss=0.5), "mirror-loss-only": dict(mirror_loss=0.5, data_augmentation=False)}
_tables = functools.partial(tables, (OD, CD, A))


def columns(dim, seed):
    """(mean, spread) per column: mean in U[-3, 3], spread log-uniform in [0.05, 20]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, dim), np.exp(rng.uniform(np.log(0.05), np.log(20.0), dim))


def constant_column(group, dim):
    """(column, value) of the group's constant column at width `dim`, or None"""
    c, v = CONSTANT[group]
    return (min(c, dim - 1), v) if dim > 1 else None


def draw(rows, group, dim, generator):
    """`rows` raw fp32 observation rows of `group` ("actor" | "critic"), `dim` wide, from its column distributions, the constant column held"""
    import torch

    mean, spread = columns(dim, STAT_SEED + (0 if group == "actor" else 1))
    x = torch.as_tensor(mean, dtype=torch.float32) + torch.as_tensor(spread, dtype=torch.float32) * torch.randn(rows, dim, generator=generator)
    if constant_column(group, dim):
        c, v = constant_column(group, dim)
        x[:, c] = v
    return x


def fit(policy):
    """the statistics: both of `policy`'s EmpiricalNormalization modules (fp32, training mode) are shown STAT_BATCHES batches of STAT_ROWS rows"""
    import torch

    from robot_lab_amd.ppo import EmpiricalNormalization

    od, cd = policy.actor[0].in_features, policy.critic[0].in_features
    g = torch.Generator().manual_seed(STAT_SEED)
    policy.train()
    for _ in range(STAT_BATCHES):
        policy.update_normalization(draw(STAT_ROWS, "actor", od, g), draw(STAT_ROWS, "critic", cd, g))
    for group, m, dim in (("actor", policy.actor_obs_normalizer, od), ("critic", policy.critic_obs_normalizer, cd)):
        if not isinstance(m, EmpiricalNormalization):  # (a policy of which only one group is normalised)
            continue
        assert m.eps == EPS and int(m.count) == STAT_BATCHES * STAT_ROWS
        if constant_column(group, dim):
            c, v = constant_column(group, dim)
            assert float(m._std[0, c]) == 0.0 and float(m._mean[0, c]) == v and int((m._std[0] == 0).sum()) == 1, "the constant column must have std = 0 exactly"
    return policy


def raw_storage(policy, seed=0, T=T, N=N):
    """`ppo_helpers.fake_storage`'s recipe (the policy's own actions; action dimension 0 positive is "good") on RAW rows of the column distributions"""
    import torch

    from robot_lab_amd.ppo import gaussian_log_prob

    od, cd = policy.actor[0].in_features, policy.critic[0].in_features
    g = torch.Generator().manual_seed(seed)
    obs, cobs = draw(T * N, "actor", od, g).reshape(T, N, od), draw(T * N, "critic", cd, g).reshape(T, N, cd)
    with torch.no_grad():
        mu, sd = policy.distribution(obs)
        act = mu + sd * torch.randn(mu.shape, generator=g)
        logp = gaussian_log_prob(act, mu, sd)
        val = policy.evaluate(cobs).squeeze(-1)
    adv = act[..., 0].clone()
    adv = (adv - adv.mean()) / adv.std()
    ret = val + adv
    return types.SimpleNamespace(num_transitions_per_env=T, num_envs=N, observations=obs, privileged_observations=cobs, actions=act, values=val.unsqueeze(-1),
                                 returns=ret.unsqueeze(-1), advantages=adv.unsqueeze(-1), actions_log_prob=logp.unsqueeze(-1), mu=mu, sigma=sd.expand_as(mu).contiguous())


@functools.lru_cache(maxsize=None)
def case(actor=True, critic=True, dims=(OD, CD, A), hidden=(512, 256, 128)):
    """(policy on the host with fitted statistics, raw storage); built once per process, read-only.  `actor` / `critic`: which groups are
    normalised; `dims`, `hidden`: another network than the A1 one"""
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pol = fit(ActorCritic(*dims, actor_hidden=hidden, critic_hidden=hidden, actor_obs_normalization=actor, critic_obs_normalization=critic))
    st = raw_storage(pol)
    g = torch.Generator().manual_seed(PERTURB_SEED)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.01 * torch.randn(p.shape, generator=g) * p.abs().mean())
    if actor and dims[0] > 1:
        assert float(pol.actor_obs_normalizer(st.observations).abs().mean()) < 2.0, "the normalised inputs of the stored rows are O(1)"
    return pol, st


def without_normalizers(pol):
    """a copy of `pol` whose normalisers are nn.Identity: the networks alone, for rows that were normalised before"""
    from torch import nn

    out = copy.deepcopy(pol)
    out.actor_obs_normalizer, out.critic_obs_normalizer = nn.Identity(), nn.Identity()
    out.actor_obs_normalization = out.critic_obs_normalization = False
    return out


def normalise(module, x):
    """THE RULE's second line on rows `x` in x's dtype: (x - mean) / (std + eps) with the module's statistics (fp32 buffers, exactly representable
    in fp64); an nn.Identity passes the rows through"""
    from robot_lab_amd.ppo import EmpiricalNormalization

    if not isinstance(module, EmpiricalNormalization):
        return x
    return (x - module._mean.to(device=x.device, dtype=x.dtype)) / (module._std.to(device=x.device, dtype=x.dtype) + module.eps)


def mirrored(x, table, n_sym):
    """THE RULE's first line: [n, dim] -> [n_sym n, dim], copy s = sign[s] * x[:, perm[s]] in rows s n .. (s + 1) n; a None table replicates"""
    import torch

    if table is None:
        return x.repeat(n_sym, 1)
    perm, sign = torch.as_tensor(table[0].astype(np.int64), device=x.device), torch.as_tensor(table[1].copy(), device=x.device).to(x.dtype)
    return torch.cat([sign[s] * x[:, perm[s]] for s in range(n_sym)], 0)


def materialise(st, tab, idx, pol, order="mirror-then-normalise"):
    """the n_sym len(idx) rows the rule is defined by, as a 1 x rows storage of NETWORK INPUTS: every raw row mirrored, then normalised with the
    statistics of the destination column (`pol`'s modules).  `tab=None`: one copy.  `order="normalise-then-mirror"`: the WRONG order (the
    teeth)."""
    import torch

    ns = tab.n_sym if tab is not None else 1
    rows_total = st.num_transitions_per_env * st.num_envs
    rows = lambda t: t.reshape(rows_total, -1)[idx]  # noqa: E731
    t_obs, t_cri, t_act = (tab.obs, tab.critic, tab.act) if tab is not None else (None, None, None)
    if order == "mirror-then-normalise":
        obs = normalise(pol.actor_obs_normalizer, mirrored(rows(st.observations), t_obs, ns))
        cobs = normalise(pol.critic_obs_normalizer, mirrored(rows(st.privileged_observations), t_cri, ns))
    else:
        obs = mirrored(normalise(pol.actor_obs_normalizer, rows(st.observations)), t_obs, ns)
        cobs = mirrored(normalise(pol.critic_obs_normalizer, rows(st.privileged_observations)), t_cri, ns)
    out = types.SimpleNamespace(num_transitions_per_env=1, num_envs=ns * len(idx))
    out.observations, out.privileged_observations, out.actions = obs, cobs, mirrored(rows(st.actions), t_act, ns)
    for k in ("values", "returns", "advantages", "actions_log_prob", "mu", "sigma"):
        setattr(out, k, rows(getattr(st, k)).repeat(ns, 1))
    for k, v in list(vars(out).items()):
        if torch.is_tensor(v):
            setattr(out, k, v.unsqueeze(0).contiguous())
    return out


def handles(pol, device=DEV):
    """(actor handle | None, critic handle | None): `ObsNormalizer`s that hold `pol`'s statistics (load_module)"""
    from robot_lab_amd.obsnorm import ObsNormalizer
    from robot_lab_amd.ppo import EmpiricalNormalization

    out = []
    for m in (pol.actor_obs_normalizer, pol.critic_obs_normalizer):
        if not isinstance(m, EmpiricalNormalization):
            out.append(None)
            continue
        h = ObsNormalizer(m._mean.shape[1], m.eps, max_rows=4096, device=device)
        h.load_module(m)
        out.append(h)
    return tuple(out)
