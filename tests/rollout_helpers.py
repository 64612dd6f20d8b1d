"""The one copy of what the rollout tests share (tests/test_rollout.py on the CPU, tests/test_gpu_rollout_exact.py on the GPU; the kernels:
robot_lab_amd/csrc/rl_rollout.hip and csrc/rollout/rl_sample.h).  numpy only.

  - the RECURSION of gae_kernel in its own operation order, in fp32 (`gae_f32`), in fp64 (`gae_f64`) and in fp32 with every a * b + c fused
    (`gae_f32_fused`, the stand-in for a kernel the compiler contracted), on done bytes in the deferred encoding of rl_env_step_record
    (0, 1 = terminated only, 3 = time out with or without termination); each returns every intermediate value;
  - fp32 EMULATIONS of the log-probability (per 4-wide Philox block, blocks summed in ascending order), of the advantage normalisation and of
    Box-Muller on the oracle's uniforms;
  - the EXACT family `exact_gae_case`: small integers times a power of two with gamma, lam in {1, 0.5} - asserted here to round nowhere,
    so any operation order and any contraction give the same bits;
  - the BOUND  max |kernel - fp64| <= K * max |fp32 emulation - fp64|, one K per group, and the regimes it is asserted in;
  - the DEFECTS that tests/test_rollout.py feeds through both (the tests' teeth).

gamma and lam enter every function as np.float32 widened to double: the C-ABI takes `float`, so 0.99 is the float nearest to it on both
sides and no reference carries the 0.99-as-double mismatch."""
import numpy as np

from oracle import philox as px
from oracle.rollout import STREAM_POLICY

F = np.float32
HALF_LOG_2PI = 0.91893853320467274178
BLOCK = 256  # threads of an act_kernel workgroup


def f32c(x):
    """a C `float` argument as the double the fp64 references use"""
    return float(np.float32(x))


def envs_per_block(act_dim):
    """act_kernel: one thread per (env, 4-wide Philox block), BLOCK / nblk envs per workgroup"""
    return BLOCK // ((act_dim + 3) // 4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_equal(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ in their bits; first at {i}: got {got[i]!r} ({bits(got)[i]:#010x}), "
                             f"want {want[i]!r} ({bits(want)[i]:#010x})")


# ---- the recursion of gae_kernel ------------------------------------------------------------------------------------------------------------
GAE_DEFECTS = ("next_v_of_step_t", "done_of_step_t_plus_1", "lam_dropped", "bit1_ignored", "bootstrap_twice", "last_values_zero", "running_a_stored")
INTERMEDIATES = ("x", "delta", "a", "returns", "advantages")


def _gae(rewards, values, dones, last_values, gamma, lam, dt, fused=False, defect=None):
    """gae_kernel, one env per column: x = (nt gamma) next_v; delta = (r + x) - v; a = delta + ((nt gamma) lam) a; ret = a + v; adv = ret - v,
    every operation rounded to `dt`; `fused`: a * b + c rounds once (through the double-precision sum of the exact product: a second rounding
    in one of ~2^29 operations).  The explicit fmaf of the time-out bootstrap is one rounding in every variant.  `defect`: one of
    GAE_DEFECTS.  Returns a dict: the INTERMEDIATES, and `rewards` / `dones` as compute_returns leaves them."""
    assert defect is None or defect in GAE_DEFECTS
    d8 = np.asarray(dones, dtype=np.uint8)
    assert np.isin(d8, (0, 1, 3)).all(), "done bytes are 0, 1 or 3"
    T, N = d8.shape
    g, lm = dt(np.float32(gamma)), dt(np.float32(lam))
    v_all, last = np.asarray(values, dtype=np.float32).astype(dt), np.asarray(last_values, dtype=np.float32).astype(dt)
    r_all = np.asarray(rewards, dtype=np.float32).astype(dt)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(dt)

    out = {k: np.zeros((T, N), dtype=dt) for k in INTERMEDIATES}
    out["rewards"], out["dones"] = r_all.copy(), (d8 != 0).astype(np.uint8)
    a = np.zeros(N, dtype=dt)
    next_v = np.zeros(N, dtype=dt) if defect == "last_values_zero" else last
    for t in range(T - 1, -1, -1):
        v, d, r = v_all[t], d8[t], r_all[t]
        boot = (d & 2) != 0
        if defect != "bit1_ignored":
            n_boot = 2 if defect == "bootstrap_twice" else 1
            for _ in range(n_boot):
                r = np.where(boot, fma(np.broadcast_to(g, v.shape), v, r), r)
        out["rewards"][t] = r
        if defect == "done_of_step_t_plus_1":
            d = d8[t + 1] if t + 1 < T else np.zeros(N, dtype=np.uint8)
        if defect == "next_v_of_step_t":
            next_v = v
        nt = np.where(d != 0, dt(0), dt(1))
        ng = nt * g
        ngl = ng if defect == "lam_dropped" else ng * lm
        if fused:
            x = ng * next_v
            delta = fma(ng, next_v, r) - v
            a = fma(ngl, a, delta)
        else:
            x = ng * next_v
            delta = (r + x) - v
            a = delta + ngl * a
        ret = a + v
        adv = a if defect == "running_a_stored" else ret - v
        for k, val in zip(INTERMEDIATES, (x, delta, a, ret, adv)):
            assert val.dtype == dt
            out[k][t] = val
        next_v = v
    return out


def gae_f32(rewards, values, dones, last_values, gamma, lam, defect=None):
    return _gae(rewards, values, dones, last_values, gamma, lam, np.float32, defect=defect)


def gae_f64(rewards, values, dones, last_values, gamma, lam):
    return _gae(rewards, values, dones, last_values, gamma, lam, np.float64)


def gae_f32_fused(rewards, values, dones, last_values, gamma, lam):
    return _gae(rewards, values, dones, last_values, gamma, lam, np.float32, fused=True)


# ---- fp32 emulations ------------------------------------------------------------------------------------------------------------------------
LOGP_DEFECTS = ("log_sigma_dropped", "last_block_dropped", "one_env_one_block_short")


def log_prob_f64(actions, mu, sigma):
    """the Gaussian log-density at the stored fp32 actions / mu / sigma, in fp64: what the learner's ratio is formed against"""
    a, m, s = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (actions, mu, sigma))
    return np.sum(-0.5 * ((a - m) / s) ** 2 - np.log(s) - HALF_LOG_2PI, axis=-1)


def log_prob_f32(actions, mu, sigma, defect=None):
    """act_block / act_kernel in fp32: per 4-wide block logp += ((-0.5 q) q - log sd) - c in ascending columns from 0, the blocks of an env
    summed in ascending order from 0.  `defect`: one of LOGP_DEFECTS (the one-env defect hits the last env of the first workgroup, or the
    last env when there is one workgroup)."""
    assert defect is None or defect in LOGP_DEFECTS
    a, m, s = (np.asarray(x, dtype=np.float32) for x in (actions, mu, sigma))
    A = a.shape[-1]
    nblk = (A + 3) // 4
    lead = a.shape[:-1]
    total = np.zeros(lead, dtype=F)
    parts = []
    for b in range(nblk):
        part = np.zeros(lead, dtype=F)
        for j in range(4 * b, min(4 * b + 4, A)):
            q = (a[..., j] - m[..., j]) / s[..., j]
            term = (F(-0.5) * q) * q
            if defect != "log_sigma_dropped":
                term = term - np.log(s[..., j])
            part = part + (term - F(HALF_LOG_2PI))
            assert part.dtype == F
        parts.append(part)
    for b, part in enumerate(parts):
        if b == nblk - 1 and nblk > 1:
            if defect == "last_block_dropped":
                continue
            if defect == "one_env_one_block_short":
                part = part.copy()
                part[..., min(envs_per_block(A), lead[-1]) - 1] = 0
        total = total + part
    return total


def normalise_f64(raw):
    x = np.asarray(raw, dtype=np.float32).astype(np.float64)
    s = x.std(ddof=1) if x.size > 1 else 0.0
    return (x - x.mean()) / (s + 1e-8)


def normalise_f32(raw, ddof=1):
    """fp32 mean and std (numpy's pairwise sums), (x - m) * (1 / (s + 1e-8)) as norm_kernel spells it.  ddof = 0: the biased-std defect"""
    x = np.asarray(raw, dtype=np.float32)
    m = x.mean(dtype=F)
    s = x.std(ddof=ddof, dtype=F) if x.size > ddof else F(0)
    out = (x - m) * (F(1) / (s + F(1e-8)))
    assert out.dtype == F
    return out


def box_muller_f32(seed, n_envs, counter, act_dim):
    """normal4 of rl_sample.h in numpy fp32 on the oracle's uniforms (24-bit, exact in fp32)"""
    env = np.arange(n_envs, dtype=np.uint32)[:, None]
    j = np.arange(act_dim, dtype=np.uint32)[None]
    pair = (j >> np.uint32(1)) << np.uint32(1)
    u_even = px.uniform(seed, env, counter, STREAM_POLICY, pair).astype(F)
    u_odd = px.uniform(seed, env, counter, STREAM_POLICY, pair + np.uint32(1)).astype(F)
    r = np.sqrt(F(-2.0) * np.log(F(1.0) - u_even))
    th = F(6.28318530717958647692) * u_odd
    z = np.where(j & np.uint32(1), r * np.sin(th), r * np.cos(th))
    assert z.dtype == F
    return z


# ---- exact family ---------------------------------------------------------------------------------------------------------------------------
def _done_bytes(rng, T, N, chain_cap, p_done):
    """done bytes 0 / 1 / 3: i.i.d. with probability p_done, or - chain_cap given - so that every chain_cap consecutive steps of an env hold
    a done (the steps behind its last done too).  Half of the dones are terminations, the other half time outs (byte 3)."""
    if chain_cap is None:
        done = rng.random((T, N)) < p_done
    else:
        done = np.zeros((T, N), dtype=bool)
        for e in range(N):
            t = int(rng.integers(0, chain_cap))
            while t < T:
                done[t, e] = True
                t += int(rng.integers(1, chain_cap + 1))
            if not done[max(0, T - chain_cap):, e].any():
                done[T - 1, e] = True
    time_out = done & (rng.random((T, N)) < 0.5)
    return (done.astype(np.uint8) | (time_out.astype(np.uint8) << 1)).astype(np.uint8), time_out


def exact_gae_case(gamma, lam, T, N, chain_cap, scale, seed, p_done=0.1):
    """Integer rewards, values and last_values in [-64, 64] times `scale`; dones i.i.d. with probability `p_done` (chain_cap None) or at
    least every `chain_cap` steps (1: every step done).  Of the time outs, half also terminate (the byte is 3 either way; the record
    kernel gets both flags).  ASSERTS the family's condition: every intermediate of gae_f32 equals gae_f64's - nothing rounds, so any
    operation order and any contraction give these bits.  Returns a dict: rewards, values, last_values (fp32), dones (bytes 0 / 1 / 3),
    terminated, time_outs (uint8 flags of the record kernel) and `want`, the fp64 recursion's result."""
    rng = np.random.default_rng(seed)
    draw = lambda *s: (rng.integers(-64, 65, s) * scale).astype(np.float32)  # noqa: E731
    rewards, values, last = draw(T, N), draw(T, N), draw(N)
    dones, time_out = _done_bytes(rng, T, N, chain_cap, p_done)
    terminated = ((dones != 0) & (~time_out | (rng.random((T, N)) < 0.5))).astype(np.uint8)
    lo, hi = gae_f32(rewards, values, dones, last, gamma, lam), gae_f64(rewards, values, dones, last, gamma, lam)
    for k in INTERMEDIATES + ("rewards",):
        assert np.array_equal(lo[k].astype(np.float64), hi[k]), f"exact_gae_case{(gamma, lam, T, N, chain_cap, scale, seed)}: {k} rounds in fp32 - not in the exact family"
    assert np.array_equal(lo["dones"], hi["dones"])
    return dict(rewards=rewards, values=values, last_values=last, dones=dones, terminated=terminated, time_outs=time_out.astype(np.uint8),
                gamma=gamma, lam=lam, want=hi)


# (gamma, lam, T, N, chain_cap, scale, p_done): the four parameter sets of the family and (1, 1) at the shapes where the kernel can go wrong
EXACT_CASES = [
    (1.0, 1.0, 24, 300, None, 1, 0.1),
    (1.0, 0.5, 24, 300, 4, 16, 0.1),
    (0.5, 0.5, 24, 300, 4, 256, 0.1),
    (0.5, 0.5, 6, 37, None, 4096, 0.1),
    (1.0, 1.0, 1, 1, None, 1, 0.1),     # T = 1, N = 1
    (1.0, 1.0, 24, 256, None, 1, 0.1),  # one full workgroup
    (1.0, 1.0, 24, 257, None, 1, 0.1),  # one thread in a second workgroup
    (1.0, 1.0, 24, 300, 1, 1, 0.1),     # every step done
    (1.0, 1.0, 24, 300, None, 1, 0.0),  # no done: chains of the whole horizon, last_values reaches step 0
]
EXACT_OUTPUTS = ("returns", "advantages", "rewards", "dones")


def exact_case(i):
    g, lm, T, N, cap, scale, p = EXACT_CASES[i]
    return exact_gae_case(g, lm, T, N, cap, scale, seed=100 + i, p_done=p)


def exact_mismatches(got, want):
    """the EXACT_OUTPUTS whose bits differ between two results of the recursion (the GPU tests assert there are none; the teeth that there are)"""
    bad = []
    for k in EXACT_OUTPUTS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        same = np.array_equal(a.astype(np.uint8), b.astype(np.uint8)) if k == "dones" else np.array_equal(bits(a), bits(b))
        if not same:
            bad.append(k)
    return bad


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------
# max |kernel - fp64 reference| <= K * max |fp32 emulation - fp64 reference| over a case.  Each K is the next power of two at or above twice the
# largest ratio measured on the MI355X in its group (profiles/rollout_accuracy.txt), never above 8.
K_GAE = 2.0    # largest measured ratio 1.000
K_NORM = 2.0   # 1.000
K_LOGP = 8.0   # 2.037 (one-wide actions, 300 envs)
K_DRAWS = 2.0  # 1.000
K_CAP = 8.0


def error_ratio(got, emu, ref):
    """(E, E32): max |got - ref| and max |emu - ref|, both against the fp64 reference"""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got).astype(np.float64) - ref).max()), float(np.abs(np.asarray(emu).astype(np.float64) - ref).max())


def check_bound(case, output, got, emu, ref, K):
    """prints the profile's line, returns (within the bound, E / E32); asserts the yardstick is not zero"""
    e, e32 = error_ratio(got, emu, ref)
    assert e32 > 0.0, f"{case} {output}: the fp32 emulation is exact here - no yardstick"
    print(f"[rollout-accuracy] {case} {output} {e:.3e} {e32:.3e} {e / e32:.3f}")
    return e <= K * e32, e / e32


def assert_bound(case, output, got, emu, ref, K):
    ok, ratio = check_bound(case, output, got, emu, ref, K)
    assert ok, f"{case} {output}: max |err| is {ratio:.2f} x the fp32 emulation's (bound {K:g} x)"
    return ratio


def gae_regime(name):
    """the GAE regimes of the bound tier: dict(rewards, values, last_values, dones (bytes 0 / 1 / 3), terminated, time_outs, gamma, lam)"""
    rng = np.random.default_rng({"production": 11, "long_chains": 12, "cancelling": 13}[name])
    if name == "production":
        T, N, g, lm = 24, 300, 0.99, 0.95
        v, last, r = 3.0 * rng.standard_normal((T, N)), 3.0 * rng.standard_normal(N), rng.standard_normal((T, N))
        term, to = rng.random((T, N)) < 0.05, rng.random((T, N)) < 0.03
    elif name == "long_chains":
        T, N, g, lm = 64, 37, 0.999, 1.0
        v, last, r = 3.0 * rng.standard_normal((T, N)), 3.0 * rng.standard_normal(N), rng.standard_normal((T, N))
        term = to = np.zeros((T, N), dtype=bool)
    else:
        T, N, g, lm = 24, 300, 0.99, 0.95
        v, last, r = 100.0 + 0.01 * rng.standard_normal((T, N)), 100.0 + 0.01 * rng.standard_normal(N), 0.01 * rng.standard_normal((T, N))
        term, to = rng.random((T, N)) < 0.05, rng.random((T, N)) < 0.03
    dones = ((term | to).astype(np.uint8) | (to.astype(np.uint8) << 1)).astype(np.uint8)
    return dict(rewards=r.astype(F), values=v.astype(F), last_values=last.astype(F), dones=dones, terminated=term.astype(np.uint8),
                time_outs=to.astype(np.uint8), gamma=g, lam=lm)


GAE_REGIMES = ("production", "long_chains", "cancelling")
GAE_BOUND_OUTPUTS = ("rewards", "returns", "advantages")


def gae_refs(c):
    """(fp32 emulation, fp64 reference) of a case dict"""
    args = (c["rewards"], c["values"], c["dones"], c["last_values"], c["gamma"], c["lam"])
    return gae_f32(*args), gae_f64(*args)


def norm_regime(name):
    """raw advantages [T, N] of the normalisation regimes that do not come out of a GAE regime.  The tests store them as rewards of a storage
    whose every step is done and whose values are zero: gae_kernel then returns them unchanged (a = r - 0, (a + 0) - 0)."""
    rng = np.random.default_rng({"mean_1000_std": 21, "tiny": 22, "two": 23}[name])
    if name == "mean_1000_std":
        # both (float)mean of the kernel and numpy's fp32 mean sit on the 6e-5 grid of fp32 near 1000: each side's error is how this seed's mean
        # happens to round there, so the measured ratio (0.917) belongs to the seed, not to the kernel.  The kernel sums in fp64 and rounds once,
        # the yardstick sums in fp32: over seeds the kernel can only be the better one.  A reseed that moves the ratio is no regression.
        return (1000.0 + rng.standard_normal((4, 37))).astype(F)
    if name == "tiny":
        return (1e-6 * rng.standard_normal((4, 37))).astype(F)
    return rng.standard_normal((2, 1)).astype(F)


NORM_REGIMES = ("mean_1000_std", "tiny", "two")


def logp_regime(name, N, A, seed):
    """(mean [N, A], std [A]) of the log-probability regimes"""
    rng = np.random.default_rng(seed)
    if name == "production":
        return rng.standard_normal((N, A)).astype(F), np.exp(rng.uniform(-1.0, 0.3, A)).astype(F)
    if name == "narrow":
        return rng.uniform(-10.0, 10.0, (N, A)).astype(F), rng.uniform(0.01, 0.05, A).astype(F)
    return rng.standard_normal((N, A)).astype(F), np.full(A, 4.0, dtype=F)


def sample_f32(mean, std, seed, counter):
    """act_block's action on the CPU: fmaf(sd, z, m) on the fp32 Box-Muller draws (the teeth need stored actions without a GPU)"""
    mean = np.asarray(mean, dtype=F)
    z = box_muller_f32(seed, mean.shape[0], counter, mean.shape[1])
    return (np.asarray(std, dtype=F).astype(np.float64) * z.astype(np.float64) + mean.astype(np.float64)).astype(F)


LOGP_REGIMES = ("production", "narrow", "sigma4")
LOGP_WIDTHS = (1, 4, 5, 12, 29, 64)
LOGP_ENVS = (37, 300)
