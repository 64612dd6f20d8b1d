"""The one copy of what the recurrent-policy tests share (tests/test_recurrent.py, tests/test_lstm_abi.py on the CPU,
tests/test_gpu_lstm_exact.py, tests/test_gpu_recurrent.py on the GPU; the kernel: robot_lab_amd/csrc/rl_lstm.hip, the rule:
robot_lab_amd/recurrent.py):

  - the fp64 cell and recursion, and the fp32 numpy EMULATION of the cell whose distance from fp64 scales the GPU bounds;
  - the INTEGER family: integer weights, inputs and states whose every partial sum of z is below 2^24 (asserted in int64 before
    anything runs), so `gates_out` equals the int64 z exactly whatever the order of the sums;
  - the SATURATED family: biases +-200 and weights that keep |z| >= 128, so every gate is exactly 0, 1 or +-1;
  - the tile edges of the kernel as built, and the bound e <= max(M_BOUND d, floor) of the learner tests (tests/ppo_helpers.py).

`torch` is imported inside the functions: the module imports wherever its users do."""
import numpy as np

from policy_helpers import M_BOUND, SPAN

DEV = "cuda:0"

# the kernel as built (csrc/rl_lstm.hip): 32 rows per workgroup in two 16-row MFMA tiles, 16-deep k blocks of x and of h (each padded on
# its own), 16 hidden units per wavefront pass, 8 wavefronts per workgroup (128 hidden units per round of passes)
ROW_TILE, ROWS_PER_WG, K_BLOCK, UNIT_TILE, UNITS_PER_ROUND = 16, 32, 16, 16, 128
ROW_EDGES = (15, 16, 17, 31, 32, 33)
D_EDGES = (15, 16, 17)          # k-block edge of the x segment
H_EDGES = (15, 16, 17, 127, 128, 129)  # k-block / unit-tile edge, and the edge of one round of the workgroup's wavefronts


def sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, dtype=np.float64)))


def cell64(x, h, c, w_ih, w_hh, b_ih, b_hh, reset=None):
    """one step in float64: (h', c', z, h~, c~)"""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    h, c = f(h), f(c)
    if reset is not None:
        keep = ~np.asarray(reset, dtype=bool)[:, None]
        h, c = np.where(keep, h, 0.0), np.where(keep, c, 0.0)
    z = f(x) @ f(w_ih).T + h @ f(w_hh).T + f(b_ih) + f(b_hh)
    H = h.shape[1]
    i, fg, g, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
    cn = sigmoid64(fg) * c + sigmoid64(i) * np.tanh(g)
    return sigmoid64(o) * np.tanh(cn), cn, z, h, c


def sigmoid32(v):
    """1 / (1 + e^-v) in float32: e^-v overflows to inf (quotient exactly 0) or underflows to 0 (quotient exactly 1)"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore"):
        out = np.float32(1) / (np.float32(1) + np.exp(-v))
    assert out.dtype == np.float32
    return out


def tanh32(v):
    return np.tanh(np.asarray(v, dtype=np.float32))


def tanh32_naive(v):
    """(e^2v - 1) / (e^2v + 1) in float32: inf / inf at v = 200 - what the saturation properties must catch"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.float32(2) * v)
        return (e - np.float32(1)) / (e + np.float32(1))


def cell32(x, h, c, w_ih, w_hh, b_ih, b_hh, reset=None, tanh=tanh32):
    """the fp32 numpy emulation of the cell: float32 operands, sums and nonlinearities; (h', c', z, h~, c~)"""
    f = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    h, c = f(h), f(c)
    if reset is not None:
        keep = ~np.asarray(reset, dtype=bool)[:, None]
        h, c = np.where(keep, h, np.float32(0)), np.where(keep, c, np.float32(0))
    z = (f(x) @ f(w_ih).T + h @ f(w_hh).T) + (f(b_ih) + f(b_hh))
    assert z.dtype == np.float32
    H = h.shape[1]
    i, fg, g, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
    cn = sigmoid32(fg) * c + sigmoid32(i) * tanh(g)
    hn = sigmoid32(o) * tanh(cn)
    return hn.astype(np.float32), cn.astype(np.float32), z, h, c


def unroll(cell, xs, resets, params, h0, c0):
    """T steps of `cell` from (h0, c0): dict of the saved states [T, N, H] (the state each step saw), the final state and the last z"""
    h, c, hs, cs, z = h0, c0, [], [], None
    for t in range(xs.shape[0]):
        h, c, z, ht, ct = cell(xs[t], h, c, *params, reset=resets[t])
        hs.append(ht)
        cs.append(ct)
    return dict(h_saved=np.stack(hs), c_saved=np.stack(cs), h=h, c=c, z=z)


def lstm_default_init(D, H, seed):
    """nn.LSTM's default initialisation: every tensor U(-1 / sqrt(H), 1 / sqrt(H))"""
    rng, k = np.random.default_rng(seed), 1.0 / np.sqrt(H)
    u = lambda *s: rng.uniform(-k, k, s).astype(np.float32)  # noqa: E731
    return u(4 * H, D), u(4 * H, H), u(4 * H), u(4 * H)


def integer_case(N, D, H, seed):
    """Integer x, h, c and parameters with sum |x| |w_ih| + sum |h| |w_hh| + |b_ih| + |b_hh| < 2^24 for every gate of every row (asserted
    in int64): every partial sum of z, in any order, is exact in fp32.  Returns float32 arrays and the int64 z [N, 4H]."""
    rng = np.random.default_rng(seed)
    # magnitudes sized so that the span holds with room: (D + H) * mx * mw <= 2^23
    mw = 7
    mx = int(max(1, min(4000, (1 << 23) // ((D + H) * mw))))
    x, h = rng.integers(-mx, mx + 1, (N, D)), rng.integers(-mx, mx + 1, (N, H))
    c = rng.integers(-3, 4, (N, H))
    w_ih, w_hh = rng.integers(-mw, mw + 1, (4 * H, D)), rng.integers(-mw, mw + 1, (4 * H, H))
    b_ih, b_hh = rng.integers(-1000, 1001, 4 * H), rng.integers(-1000, 1001, 4 * H)
    span = np.abs(x).astype(np.int64) @ np.abs(w_ih).T.astype(np.int64) + np.abs(h).astype(np.int64) @ np.abs(w_hh).T.astype(np.int64) + np.abs(b_ih) + np.abs(b_hh)
    assert span.dtype == np.int64 and span.max() < SPAN, f"sum |x| |w| + |b| reaches {span.max()} >= 2^24"
    z = x.astype(np.int64) @ w_ih.T.astype(np.int64) + h.astype(np.int64) @ w_hh.T.astype(np.int64) + b_ih + b_hh
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return f(x), f(h), f(c), (f(w_ih), f(w_hh), f(b_ih), f(b_hh)), z


# the integer cases: (N, D, H) - the sizes the issue names plus one below / at / one above every row, k and unit tile edge of the kernel
INTEGER_CASES = [
    (1, 1, 1), (15, 3, 4), (16, 45, 20), (17, 235, 64), (64, 512, 256), (257, 45, 256),
    (31, 15, 15), (32, 16, 16), (33, 17, 17), (15, 16, 127), (16, 17, 128), (17, 15, 129), (33, 512, 512), (64, 1, 20),
]


def saturated_case(N, D, H, seed):
    """Biases +-200 (b_ih carries them, b_hh = 0), |x|, |h| <= 1 and weights small enough that |W x| + |W h| <= 72: |z| >= 128 everywhere, so
    every sigmoid is exactly 0 or 1 and tanh(z_g) exactly +-1.  One parameter set per gate pattern (same weights, other biases):
    "hold" f = 1, i = 0, o = 0;  "write+" / "write-" f = 0, i = 1, o = 1, g = +-1.  c is non-zero (0.25 <= |c| <= 4), both signs."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (N, D)).astype(np.float32)
    h = rng.uniform(-1, 1, (N, H)).astype(np.float32)
    c = rng.uniform(0.25, 4.0, (N, H)).astype(np.float32) * rng.choice([-1.0, 1.0], (N, H)).astype(np.float32)
    lim = 36.0
    w_ih = rng.uniform(-lim / D, lim / D, (4 * H, D)).astype(np.float32)
    w_hh = rng.uniform(-lim / H, lim / H, (4 * H, H)).astype(np.float32)
    params = {}
    for k, (bi, bf, bg, bo) in {"hold": (-200, 200, 200, -200), "write+": (200, -200, 200, 200), "write-": (200, -200, -200, 200)}.items():
        b = np.concatenate([np.full(H, v, dtype=np.float32) for v in (bi, bf, bg, bo)])
        params[k] = (w_ih, w_hh, b, np.zeros(4 * H, dtype=np.float32))
    zmax = np.abs(x.astype(np.float64)) @ np.abs(w_ih.astype(np.float64)).T + np.abs(h.astype(np.float64)) @ np.abs(w_hh.astype(np.float64)).T
    assert zmax.max() <= 72.0, zmax.max()
    return x, h, c, params


def bound_check(name, got, ref64, emu32, lines=None):
    """e <= max(M_BOUND d, floor): e, d the max errors of the kernel and of the fp32 emulation against fp64, relative to max |ref64|; floor one
    fp32 spacing of that maximum (tests/ppo_helpers.py's convention).  Returns (ok, line)."""
    ref64 = np.asarray(ref64, dtype=np.float64)
    scale = float(np.abs(ref64).max()) or 1.0
    e = float(np.abs(np.asarray(got, dtype=np.float64) - ref64).max()) / scale
    d = float(np.abs(np.asarray(emu32, dtype=np.float64) - ref64).max()) / scale
    floor = float(np.spacing(np.float32(scale))) / scale
    line = f"{name:<34}{scale:12.4e}{e:12.3e}{d:12.3e}{(e / d if d else float('inf')):8.2f}{floor:12.3e}"
    print(line)
    if lines is not None:
        lines.append(line)
    return e <= max(M_BOUND * d, floor), line


BOUND_HEADER = f"{'case / tensor':<34}{'max|ref64|':>12}{'e (hip)':>12}{'d (numpy32)':>12}{'e/d':>8}{'floor':>12}"
BOUND_CASES = [(45, 256), (235, 256), (7, 20)]  # (D, H), N = 256, 24 steps
BOUND_ROWS, BOUND_STEPS = 256, 24


def bound_case(D, H, seed=0):
    """nn.LSTM's default initialisation, x ~ N(0, 1), resets on about a tenth of the (row, step) pairs"""
    rng = np.random.default_rng(100 + seed)
    params = lstm_default_init(D, H, seed)
    xs = rng.standard_normal((BOUND_STEPS, BOUND_ROWS, D)).astype(np.float32)
    resets = rng.random((BOUND_STEPS, BOUND_ROWS)) < 0.1
    return params, xs, resets


# ---- the rule: the test's own split-and-pad implementation -------------------------------------------------------------------------
def split_and_pad_unroll(policy, obs, cobs, hidden_a, hidden_c, dones):
    """The update's forward WITHOUT masks: every env's T steps are cut behind each done into trajectories, the trajectories are padded to T
    and run through `nn.LSTM` itself as one batch - the first trajectory of an env from the saved state, every later one from zero -, and the
    valid outputs are put back in [T, n] order.  Returns (mean [T, n, A], value [T, n])."""
    import torch

    T, n = dones.shape
    outs = []
    for mem, x, (h0, c0) in ((policy.memory_a, obs, hidden_a), (policy.memory_c, cobs, hidden_c)):
        trajs, starts, owners = [], [], []
        for e in range(n):
            t0 = 0
            for t in range(T):
                if dones[t, e] or t == T - 1:
                    trajs.append(x[t0:t + 1, e])
                    starts.append(t0)
                    owners.append(e)
                    t0 = t + 1
            assert t0 == T
        padded = torch.zeros(T, len(trajs), x.shape[-1], dtype=x.dtype)
        for k, tr in enumerate(trajs):
            padded[:tr.shape[0], k] = tr
        H = h0.shape[-1]
        hs = torch.stack([h0[e] if s == 0 else torch.zeros(H, dtype=x.dtype) for e, s in zip(owners, starts)]).unsqueeze(0)
        cs = torch.stack([c0[e] if s == 0 else torch.zeros(H, dtype=x.dtype) for e, s in zip(owners, starts)]).unsqueeze(0)
        y, _ = mem.rnn(padded, (hs, cs))
        rows = [[None] * n for _ in range(T)]
        for k, (tr, s, e) in enumerate(zip(trajs, starts, owners)):
            for j in range(tr.shape[0]):
                rows[s + j][e] = y[j, k]
        outs.append(torch.stack([torch.stack(r) for r in rows]))
    return policy.actor(outs[0]), policy.critic(outs[1]).squeeze(-1)


def rule_case(seed=0, T=6, N=5, H=3, D=4, Dc=5, A=2):
    """The CPU rule test's batch in fp64: dones at t = 0 (env 0), at T - 1 (env 1), twice in a row (env 2), in no step (env 3); env 4 is the
    remainder of two mini-batches and carries one done too."""
    import types

    import torch

    from robot_lab_amd.recurrent import ActorCriticRecurrent

    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    torch.manual_seed(seed)
    policy = ActorCriticRecurrent(D, Dc, A, actor_hidden=(8,), critic_hidden=(8,), rnn_hidden_dim=H).double()
    dones = torch.zeros(T, N, dtype=torch.bool)
    dones[0, 0] = True
    dones[T - 1, 1] = True
    dones[2, 2] = dones[3, 2] = True
    dones[1, 4] = True
    mu = r(T, N, A)
    sigma = torch.full((T, N, A), 0.8, dtype=torch.float64)
    actions = mu + 0.8 * r(T, N, A)
    from robot_lab_amd.ppo import gaussian_log_prob

    st = types.SimpleNamespace(num_envs=N, num_transitions_per_env=T, observations=r(T, N, D), privileged_observations=r(T, N, Dc), actions=actions, mu=mu, sigma=sigma,
                               actions_log_prob=gaussian_log_prob(actions, mu, sigma), values=r(T, N), returns=r(T, N), advantages=r(T, N), dones=dones,
                               hidden_a=(0.5 * r(N, H), 0.5 * r(N, H)), hidden_c=(0.5 * r(N, H), 0.5 * r(N, H)))
    return policy, st


# ---- the two spellings of a recurrent runner cfg (robot_lab_amd.recurrent.read_recurrent_cfg) -------------------------------------------
RSL_RL_SPELLING = dict(policy=dict(class_name="ActorCriticRecurrent", init_noise_std=0.8, actor_hidden_dims=[128, 128, 128], critic_hidden_dims=[128, 128, 64],
                                   activation="elu", rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1),
                       algorithm=dict(class_name="PPO"), obs_groups={"policy": ["policy"], "critic": ["critic"]})
_RNN = dict(class_name="RNNModel", activation="elu", obs_normalization=False, rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)
REFERENCE_SPELLING = dict(actor=dict(hidden_dims=[128, 128, 128], distribution_cfg=dict(class_name="GaussianDistribution", init_std=0.8), **_RNN),
                          critic=dict(hidden_dims=[128, 128, 64], **_RNN), algorithm=dict(class_name="PPO"),
                          obs_groups={"actor": ["policy"], "critic": ["critic"]})
