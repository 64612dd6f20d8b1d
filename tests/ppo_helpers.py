"""The one copy of what the PPO learner tests share (tests/test_ppo*.py on the CPU, tests/test_gpu_ppo_hip*.py on the GPU): the synthetic batch,
the batch designed to reach every branch of the loss head (`branch_storage`, its classes and census), the storage on the device, random symmetry tables, the torch learner that records its learning-rate path, and the gradient bound
e <= max(8 d, floor).  `torch` is imported inside the functions: the module imports wherever its users do."""
import copy
import functools
import types

import numpy as np

DEV = "cuda:0"


def fake_storage(policy, T=8, N=64, od=10, cd=14, A=3, seed=0, dtype=None):
    """a synthetic T x N batch of `policy`'s own actions in which action dimension 0 being positive is "good": the update must raise the
    policy's mean along it.  `dtype`: of the drawn numbers (None: torch's default, fp32)"""
    import torch

    from robot_lab_amd.ppo import gaussian_log_prob

    g = torch.Generator().manual_seed(seed)
    obs, cobs = torch.randn(T, N, od, generator=g, dtype=dtype), torch.randn(T, N, cd, generator=g, dtype=dtype)
    with torch.no_grad():
        mu, sd = policy.distribution(obs)
        act = mu + sd * torch.randn(mu.shape, generator=g, dtype=dtype)
        logp = gaussian_log_prob(act, mu, sd)
        val = policy.critic(cobs).squeeze(-1)
    adv = act[..., 0].clone()
    adv = (adv - adv.mean()) / adv.std()
    ret = val + adv
    return types.SimpleNamespace(num_transitions_per_env=T, num_envs=N, observations=obs, privileged_observations=cobs, actions=act, values=val.unsqueeze(-1),
                                 returns=ret.unsqueeze(-1), advantages=adv.unsqueeze(-1), actions_log_prob=logp.unsqueeze(-1), mu=mu, sigma=sd.expand_as(mu).contiguous())


SUR = ("tie", "t1 > t2", "t1 < t2")  # the outcomes of ppo_head_kernel's surrogate: in-band (or adv == 0), the unclipped term, the clamped one
VAL = ("in-band", "dv > clip, l1 > l2", "dv > clip, l1 < l2", "dv < -clip, l1 > l2", "dv < -clip, l1 < l2")
COMBO = ("adv > 0, r < lo", "adv < 0, r < lo", "adv > 0, r > hi", "adv < 0, r > hi")
MARGIN = 0.01  # no row nearer than this to a switch of the loss head: the HIP forward is ~1e-6 from fp64, so both sides take the same branch


def branch_classes(policy, st, clip=0.2, symmetry=None):
    """Which branch of the loss head every row of `st` takes, from the fp64 forward of `policy` alone (never from the code under test):
    `sur` indexes SUR, `val` VAL, `combo` COMBO (-1: in-band or adv == 0); `margin_r`, `margin_dv`, `margin_ret` are the row's distances
    |r - (1 +- clip)|, ||dv| - clip| and |ret - (v + vc) / 2| from the three switches.  `symmetry`: the classes of the n_sym n virtual rows,
    copy s in rows s n .. (s + 1) n, observations and actions mirrored, the stored terms repeated."""
    import torch

    from robot_lab_amd.ppo import gaussian_log_prob

    p64 = copy.deepcopy(policy).double().cpu()
    B = st.num_transitions_per_env * st.num_envs
    obs, cobs, act = (getattr(st, k).reshape(B, -1).double().cpu() for k in ("observations", "privileged_observations", "actions"))
    vo, ret, adv, lp_old = (getattr(st, k).reshape(B).double().cpu() for k in ("values", "returns", "advantages", "actions_log_prob"))
    if symmetry is not None:
        def mirrored(x, table):
            if table is None:
                return x.repeat(symmetry.n_sym, 1)
            return torch.cat([torch.as_tensor(table[1][s].copy()).double() * x[:, torch.as_tensor(table[0][s].astype(np.int64))] for s in range(symmetry.n_sym)], 0)

        obs, cobs, act = mirrored(obs, symmetry.obs), mirrored(cobs, symmetry.critic), mirrored(act, symmetry.act)
        vo, ret, adv, lp_old = (x.repeat(symmetry.n_sym) for x in (vo, ret, adv, lp_old))
    with torch.no_grad():
        mean, std = p64.distribution(obs)
        r = torch.exp(gaussian_log_prob(act, mean, std) - lp_old)
        v = p64.critic(cobs).view(-1)
    lo, hi = 1.0 - clip, 1.0 + clip
    t1, t2 = -adv * r, -adv * r.clamp(lo, hi)
    dv = v - vo
    vc = vo + dv.clamp(-clip, clip)
    l1, l2 = (v - ret) ** 2, (vc - ret) ** 2
    side = (dv > clip).long() - (dv < -clip).long()
    c = types.SimpleNamespace(rows=r.numel(), r=r, adv=adv, dv=dv)
    c.sur = (t1 > t2).long() + 2 * (t1 < t2).long()
    c.combo = torch.where((adv != 0) & ((r < lo) | (r > hi)), (adv < 0).long() + 2 * (r > hi).long(), torch.full_like(c.sur, -1))
    c.val = torch.where(side == 0, torch.zeros_like(side), torch.where(side > 0, 1, 3) + (l1 < l2).long())
    c.margin_r = torch.minimum((r - lo).abs(), (r - hi).abs())
    c.margin_dv = (dv.abs() - clip).abs()
    c.margin_ret = (ret - 0.5 * (v + vc)).abs()
    return c


def branch_census(c):
    """{class name: its share of the rows} of `branch_classes`' result; `zero advantage` is reported beside the classes"""
    out = {f"surrogate {n}": float((c.sur == i).double().mean()) for i, n in enumerate(SUR)}
    out.update({n: float((c.combo == i).double().mean()) for i, n in enumerate(COMBO)})
    out.update({f"value {n}": float((c.val == i).double().mean()) for i, n in enumerate(VAL)})
    out["zero advantage"] = float((c.adv == 0).double().mean())
    return out


def check_branches(title, c, share=0.10):
    """prints the census and the margins, asserts every class >= `share` of the rows (None: margins only) and every margin >= MARGIN"""
    census = branch_census(c)
    margins = {k: float(getattr(c, k).min()) for k in ("margin_r", "margin_dv", "margin_ret")}
    print(f"\n{title}: {c.rows} rows, r {float(c.r.min()):.3f} .. {float(c.r.max()):.3f}, max|dv| {float(c.dv.abs().max()):.3f}")
    for k, v in census.items():
        print(f"  {k:<30}{100 * v:6.1f} %")
    print("  smallest margins: " + ", ".join(f"{k[7:]} {v:.4f}" for k, v in margins.items()))
    assert all(v >= MARGIN for v in margins.values()), f"{title}: a row sits within {MARGIN} of a switch of the loss head: {margins}"
    if share is not None:
        low = {k: v for k, v in census.items() if k != "zero advantage" and v < share}
        assert not low and census["zero advantage"] > 0, f"{title}: classes below {share:.0%} of the rows: {low}"
    return census


def branch_storage(policy, rows, od, cd, A, seed, clip=0.2):
    """`fake_storage`'s observations and actions (1 x rows) with the stored terms set from the fp64 forward of `policy`, so that every row's branch
    of the loss head is fixed by construction - returns (storage, `branch_classes` of it).
      actions_log_prob  log-prob - log r; r in U(0.85, 1.15), below the band in U(0.3, 0.75) or above it in U(1.25, 2.5)
      advantages        +-(0.2 + |fake_storage's|), the sign by class, so that each side of the band meets both signs; exactly 0 in one row of 29
      values            value - dv; |dv| in U(0.02, 0.15), dv in U(0.25, 0.6) or -dv in U(0.25, 0.6)
      returns           clipped rows: below min(v, vc) or above max(v, vc) by U(0.05, 0.5) - l1 > l2 and l1 < l2 for either sign of dv; in-band
                        rows: values + advantages
      mu, sigma         moved off the current distribution (mu by 0.1 sigma randn, sigma by U(0.85, 1.15)): a KL of about 0.0125 per action,
                        well above twice the default desired_kl at either shape
    Classes cycle with the row number (periods 6 and 5), so the census holds at any row count.  The stored numbers are fp32, as the learners read
    them; the classes and margins are those of the rounded numbers."""
    import torch

    from robot_lab_amd.ppo import gaussian_log_prob

    st = fake_storage(policy, 1, rows, od, cd, A, seed)
    p64 = copy.deepcopy(policy).double()
    g = torch.Generator().manual_seed(seed + 1000)
    u = lambda a, b: a + (b - a) * torch.rand(rows, generator=g, dtype=torch.float64)  # noqa: E731
    i = torch.arange(rows)
    with torch.no_grad():
        mean, std = p64.distribution(st.observations.reshape(rows, od).double())
        logp = gaussian_log_prob(st.actions.reshape(rows, A).double(), mean, std)
        v = p64.critic(st.privileged_observations.reshape(rows, cd).double()).view(-1)
    # surrogate: (side of the band, sign of the advantage) by row number
    side = torch.tensor([0, -1, -1, 1, 1, 0])[i % 6]
    sign = torch.tensor([1.0, 1.0, -1.0, 1.0, -1.0, -1.0], dtype=torch.float64)[i % 6]
    r = torch.where(side == 0, u(0.85, 1.15), torch.where(side < 0, u(0.3, 0.75), u(1.25, 2.5)))
    adv = sign * (0.2 + st.advantages.reshape(rows).double().abs())
    adv[i % 29 == 7] = 0.0
    # value: (side of dv, which of l1 / l2 is larger) by row number
    vcls = i % 5
    mag, dsign = u(0.25, 0.6), torch.where(u(0.0, 1.0) < 0.5, -1.0, 1.0)
    dv = torch.where(vcls == 0, dsign * u(0.02, 0.15), torch.where(vcls <= 2, mag, -mag))
    vo = v - dv
    vc = vo + dv.clamp(-clip, clip)
    off = u(0.05, 0.5)
    below, above = torch.minimum(v, vc) - off, torch.maximum(v, vc) + off
    ret = torch.where(vcls == 0, vo + adv, torch.where((vcls == 1) | (vcls == 4), below, above))  # (nearer vc: l1 > l2)
    mu = mean + 0.1 * std * torch.randn(mean.shape, generator=g, dtype=torch.float64)
    sigma = std * (0.85 + 0.3 * torch.rand(mean.shape, generator=g, dtype=torch.float64))
    f32 = lambda t, shape: t.float().reshape(shape).contiguous()  # noqa: E731
    st.actions_log_prob, st.advantages = f32(logp - torch.log(r), (1, rows, 1)), f32(adv, (1, rows, 1))
    st.values, st.returns = f32(vo, (1, rows, 1)), f32(ret, (1, rows, 1))
    st.mu, st.sigma = f32(mu, (1, rows, A)), f32(sigma, (1, rows, A))
    return st, branch_classes(policy, st, clip)


def perturb(pol, seed=1, scale=0.01):
    """every parameter moved by `scale` randn mean|p|, in place: no two entries of std equal, no bias zero"""
    import torch

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(scale * torch.randn(p.shape, generator=g) * p.abs().mean())
    return pol


# the two shapes of tests/test_gpu_ppo_hip_branches.py (and of the CPU checks of the batch in tests/test_ppo.py): the A1 network on 1000 rows - no
# multiple of any tile - and a small odd network on 37.  `seed`: of the batch; with the 37-row one every VIRTUAL row under tables((19, 23, 5), 2)
# keeps the margins too (its copy-1 rows land where the mirrored forward puts them: checked, not constructed)
BRANCH_SHAPES = {"a1-1000": dict(dims=(45, 235, 12), hidden=(512, 256, 128), rows=1000, seed=3),
                 "odd-37": dict(dims=(19, 23, 5), hidden=(40, 24), rows=37, seed=12)}


@functools.lru_cache(maxsize=None)
def branch_case(name):
    """(policy on the host, designed storage, classes) of BRANCH_SHAPES[name]; built once per process, read-only"""
    import torch

    from robot_lab_amd.ppo import ActorCritic

    s = BRANCH_SHAPES[name]
    torch.manual_seed(0)
    pol = perturb(ActorCritic(*s["dims"], actor_hidden=s["hidden"], critic_hidden=s["hidden"]))
    st, cls = branch_storage(pol, s["rows"], *s["dims"], seed=s["seed"])
    return pol, st, cls


def reference_gradients(pol, st, device=None, **kw):
    """{dtype: {parameter name: gradient, fp64 on the host}} and {dtype: the learner} of the unchanged `ppo.PPO` in fp64 and fp32: one epoch of one
    mini-batch over `st` with a clipping norm so large that `clip_grad_norm_` multiplies by 1"""
    import torch

    ref, algs = {}, {}
    for dtype in (torch.float64, torch.float32):
        alg = torch_learner(pol, dtype, device, **dict(dict(num_learning_epochs=1, num_mini_batches=1, max_grad_norm=1e30), **kw))
        alg.update(cast(st, dtype, device=device), torch.Generator(device=device or DEV).manual_seed(5))
        ref[dtype], algs[dtype] = {n: p.grad.detach().double().cpu() for n, p in alg.policy.named_parameters()}, alg
    return ref, algs


def cast(st, dtype, rows=None, device=None):
    """the storage on the device (`device`: another one) in `dtype`; `rows`: only these rows of the flat batch, as a 1 x len(rows) storage - one
    epoch of one mini-batch of the torch learner is then the gradient on them"""
    import torch

    out = types.SimpleNamespace(num_transitions_per_env=st.num_transitions_per_env, num_envs=st.num_envs)
    for k, v in vars(st).items():
        if torch.is_tensor(v):
            v = v.to(device=device or DEV, dtype=dtype)
            if rows is not None:
                v = v.reshape(st.num_transitions_per_env * st.num_envs, -1)[rows].unsqueeze(0).contiguous()
            setattr(out, k, v)
    if rows is not None:
        out.num_transitions_per_env, out.num_envs = 1, len(rows)
    return out


def random_table(rng, n_sym, dim):
    """random signed permutations, row 0 the identity: arbitrary gathers, independent of symmetry.py's builders"""
    perm = np.stack([np.arange(dim)] + [rng.permutation(dim) for _ in range(n_sym - 1)]).astype(np.int32)
    sign = np.concatenate([np.ones((1, dim)), rng.choice([-1.0, 1.0], size=(n_sym - 1, dim))]).astype(np.float32)
    return perm, sign


def tables(dims, n_sym, critic=True, seed=11):
    """SymmetryTables of random tables for dims = (obs, critic obs, action) widths; `critic=False`: the critic's rows replicated"""
    from robot_lab_amd.symmetry import SymmetryTables

    rng = np.random.default_rng(seed)
    obs, cri, act = (random_table(rng, n_sym, d) for d in dims)
    return SymmetryTables(obs=obs, critic=cri if critic else None, act=act)


def gen(seed=1):
    import torch

    return torch.Generator(device=DEV).manual_seed(seed)


def perm(rows, seed=1):
    """the permutation of `rows` rows that PPO.update draws from `gen(seed)`"""
    import torch

    return torch.randperm(rows, device=DEV, generator=gen(seed))


def torch_learner(pol, dtype, device=None, **kw):
    """the unchanged torch learner on a copy of `pol` (`device`: elsewhere than on DEV); records the learning rate in force at every optimiser step"""
    from robot_lab_amd.ppo import PPO

    p = copy.deepcopy(pol).to(device=device or DEV, dtype=dtype)
    alg = PPO(p, **kw)
    alg.lr_path = []
    step = alg.optimizer.step

    def recording_step(*a, **k):
        alg.lr_path.append(alg.optimizer.param_groups[0]["lr"])
        return step(*a, **k)

    alg.optimizer.step = recording_step
    return alg


def split(flat, pol):
    """{parameter name: its slice of the flat buffer, fp64 on the host}"""
    out, o = {}, 0
    for name, p in pol.named_parameters():
        out[name] = flat[o:o + p.numel()].double().cpu()
        o += p.numel()
    assert o == flat.numel()
    return out


def compare_gradients(title, g_hip, ref, only=None):
    """prints the table, returns the tensors above e <= max(8 d, one fp32 spacing of max|g64| relative to it)"""
    import torch

    print(f"\n{title}\n{'tensor':<18}{'max|g64|':>12}{'e (hip)':>12}{'d (torch32)':>13}{'e/d':>8}{'floor':>12}")
    bad = []
    for n, g64 in ref[torch.float64].items():
        if only is not None and not n.startswith(only):
            continue
        scale = g64.abs().max().item()
        assert scale > 0, n
        e = (g_hip[n].reshape(g64.shape) - g64).abs().max().item() / scale
        d = (ref[torch.float32][n] - g64).abs().max().item() / scale
        floor = float(np.spacing(np.float32(scale))) / scale
        print(f"{n:<18}{scale:12.4e}{e:12.3e}{d:13.3e}{e / d if d else float('inf'):8.2f}{floor:12.3e}")
        if not e <= max(8 * d, floor):
            bad.append((n, e, d, floor))
    return bad
