"""The one copy of what the PPO learner tests share (tests/test_ppo*.py on the CPU, tests/test_gpu_ppo_hip*.py on the GPU): the synthetic batch,
the storage on the device, random symmetry tables, the torch learner that records its learning-rate path, and the gradient bound
e <= max(8 d, floor).  `torch` is imported inside the functions: the module imports wherever its users do."""
import copy
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


def cast(st, dtype, rows=None):
    """the storage on the device in `dtype`; `rows`: only these rows of the flat batch, as a 1 x len(rows) storage - one epoch of one mini-batch of
    the torch learner is then the gradient on them"""
    import torch

    out = types.SimpleNamespace(num_transitions_per_env=st.num_transitions_per_env, num_envs=st.num_envs)
    for k, v in vars(st).items():
        if torch.is_tensor(v):
            v = v.to(device=DEV, dtype=dtype)
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


def torch_learner(pol, dtype, **kw):
    """the unchanged torch learner on a copy of `pol`; records the learning rate in force at every optimiser step"""
    from robot_lab_amd.ppo import PPO

    p = copy.deepcopy(pol).to(device=DEV, dtype=dtype)
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
