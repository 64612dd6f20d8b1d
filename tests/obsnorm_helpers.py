"""The one copy of what the observation-normalisation tests share (tests/test_obsnorm.py on the CPU, tests/test_gpu_obsnorm.py and
tests/test_gpu_obsnorm_train.py on the GPU; the kernels: robot_lab_amd/csrc/rl_obsnorm.hip; the rule: robot_lab_amd.ppo.EmpiricalNormalization).
numpy only.

  - THE RULE restated on numpy arrays (`rule`): the seven lines of `EmpiricalNormalization.update` in a chosen dtype, with the batch statistics
    (mean_x, var_x) from a pluggable function - `two_pass` (numpy's mean / var, as torch computes them), the fp64 reference, and the DEFECTS
    `naive_variance` (sum x^2 / n - mean^2) and `tiles(cross_term=False)` (Chan's merge of 64-row tiles without the delta^2 term);
  - the EXACT family `exact_batches`: integers in [-4, 4], some columns scaled by 2^+-10, 64 or 256 rows, one or two updates - asserted here
    in int64 / fp64 to round nowhere in fp32 (the square root aside, which fp32 and fp64-then-fp32 round alike);
  - the BOUNDED family `bounded_batches` and the bound  max |state - fp64 rule| <= K * max |fp32 numpy rule - fp64 rule|  per state vector."""
import numpy as np

F = np.float32
EPS = 1e-2
TILE = 64  # rows of a tile of update_kernel
ROWS = (1, 63, 64, 65, 257, 4096)
DIMS = (1, 3, 45, 47, 235, 512)
VECTORS = ("mean", "var", "std")


def fresh(dim, dt=np.float64):
    return dict(mean=np.zeros(dim, dt), var=np.ones(dim, dt), std=np.ones(dim, dt), count=0)


def two_pass(x, dt):
    """numpy's column mean and population variance in `dt` (pairwise sums; var = mean |x - mean|^2: two passes, as torch.var_mean)"""
    x = x.astype(dt)
    return x.mean(axis=0, dtype=dt), x.var(axis=0, dtype=dt)


def naive_variance(x, dt):
    """DEFECT: var = sum x^2 / n - mean^2, which cancels when |mean| >> std"""
    x = x.astype(dt)
    n = dt(x.shape[0])
    m = x.sum(axis=0, dtype=dt) / n
    return m, (x * x).sum(axis=0, dtype=dt) / n - m * m


def tiles(x, dt, cross_term=True):
    """per-tile two-pass (n, mean, M2), merged in tile order with Chan's formula in `dt`; `cross_term=False`: the DEFECT that adds the M2s only"""
    x = x.astype(dt)
    n = m = M2 = None
    for r0 in range(0, x.shape[0], TILE):
        t = x[r0:r0 + TILE]
        nb, mb = dt(t.shape[0]), t.sum(axis=0, dtype=dt) / dt(t.shape[0])
        qb = ((t - mb) ** 2).sum(axis=0, dtype=dt)
        if n is None:
            n, m, M2 = nb, mb, qb
            continue
        delta, tot = mb - m, n + nb
        m = m + delta * (nb / tot)
        M2 = M2 + qb + (delta * delta * (n * nb / tot) if cross_term else dt(0))
        n = tot
    return m, M2 / n


def rule(state, x, dt=np.float64, stats=two_pass, trace=None):
    """the seven lines of EmpiricalNormalization.update on a state dict (mean, var, std: [dim] of `dt`; count: int) -> the new state dict.
    `trace`: a list that receives every intermediate array (the exact family's assertion walks it)."""
    n = x.shape[0]
    count = state["count"] + n
    rate = dt(F(n) / F(count))  # the rule's one fp32 division, in every precision
    mean_x, var_x = stats(x, dt)
    delta = mean_x - state["mean"]
    mean = state["mean"] + rate * delta
    inner = delta * (mean_x - mean)
    step = rate * ((var_x - state["var"]) + inner)
    var = state["var"] + step
    if trace is not None:
        trace += [mean_x, var_x, delta, rate * delta, mean, mean_x - mean, inner, var_x - state["var"], (var_x - state["var"]) + inner, step, var]
    out = dict(mean=mean, var=var, std=np.sqrt(var), count=count)
    assert all(out[k].dtype == dt for k in VECTORS)
    return out


def replay(batches, dt=np.float64, stats=two_pass, state=None):
    state = fresh(batches[0].shape[1], dt) if state is None else state
    for x in batches:
        state = rule(state, x, dt, stats)
    return state


def apply_f32(x, mean, std, eps=EPS):
    """numpy's fp32 (x - mean) / (std + eps): three roundings"""
    out = (np.asarray(x, F) - np.asarray(mean, F)) / (np.asarray(std, F) + F(eps))
    assert out.dtype == F
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_bits_equal(got, want, what=""):
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ in their bits; first at {i}: got {got[i]!r} ({bits(got)[i]:#010x}), "
                             f"want {want[i]!r} ({bits(want)[i]:#010x})")


# ---- exact family ---------------------------------------------------------------------------------------------------------------------------
EXACT_ROWS = (64, 256)


def _holds_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(F).astype(np.float64), a))


def exact_stats(k, scale):
    """column mean and population variance of x = k * scale (k: int64 [n, dim], scale: a power of two per column, n a power of two) from
    INTEGER sums: mean = scale sum k / n, var = scale^2 (n sum k^2 - (sum k)^2) / n^2, both exact in fp64"""
    n = k.shape[0]
    assert k.dtype == np.int64 and n & (n - 1) == 0
    s, q = k.sum(axis=0), (k * k).sum(axis=0)
    return scale * (s.astype(np.float64) / n), scale * scale * ((n * q - s * s).astype(np.float64) / (n * n))


def exact_batches(n_rows, dim, updates, seed):
    """(start state, `updates` batches [n_rows, dim] of the exact family, the states the fp64 rule gives after each).  Column 0 is constant
    (variance exactly 0), every third column is scaled by s = 2^10, every fifth by s = 2^-10.  The start state is the fresh one (mean 0, var 1,
    std 1, count 0) with var = s^2, std = s in the scaled columns (the tests set it through the set call): a scaled column is then the unscaled
    computation times a power of two at every step, where against var = 1 the difference var_x - 1 would need 32 bits.  ASSERTS that every
    intermediate of the rule is an fp32 number (the rates are 1 and 1 / 2), so any summation order gives these bits."""
    assert n_rows in EXACT_ROWS and updates in (1, 2)
    rng = np.random.default_rng(seed)
    scale = np.ones(dim)
    scale[::3], scale[::5] = 2.0 ** 10, 2.0 ** -10
    start = dict(mean=np.zeros(dim), var=scale * scale, std=scale.copy(), count=0)
    batches, states, state = [], [], start
    for u in range(updates):
        k = rng.integers(-4, 5, (n_rows, dim)).astype(np.int64)
        k[:, 0] = 3
        x = (k * scale).astype(F)
        assert np.array_equal(x.astype(np.float64), k * scale)
        trace = []
        state = rule(state, x, np.float64, lambda _x, _dt: exact_stats(k, scale), trace)
        m2, v2 = two_pass(x, np.float64)
        assert np.allclose(trace[0], m2, rtol=1e-13, atol=0) and np.allclose(trace[1], v2, rtol=1e-11, atol=0)  # (the integer route is the statistic it claims to be)
        for i, a in enumerate(trace):
            assert _holds_f32(a), f"exact_batches{(n_rows, dim, updates, seed)}: intermediate {i} of update {u} rounds in fp32 - not in the exact family"
        assert F(n_rows) / F(state["count"]) in (F(1), F(0.5))
        batches.append(x)
        states.append(state)
    assert batches and state["var"][0] == 0.0
    return start, batches, states


# ---- bounded family -------------------------------------------------------------------------------------------------------------------------
def bounded_batches(n_rows, dim, updates, seed):
    """random batches whose first columns are the hard ones: mean 1e3 with std 1e-2 (column 0), mean 0 with std 1e-4 (1), constant but for one
    row (2); the rest N(mu_c, s_c^2) with mu_c in [-3, 3], s_c in [0.1, 2]"""
    rng = np.random.default_rng(seed)
    mu, sd = rng.uniform(-3, 3, dim), rng.uniform(0.1, 2.0, dim)
    out = []
    for _ in range(updates):
        x = mu + sd * rng.standard_normal((n_rows, dim))
        x[:, 0] = 1e3 + 1e-2 * rng.standard_normal(n_rows)
        if dim > 1:
            x[:, 1] = 1e-4 * rng.standard_normal(n_rows)
        if dim > 2:
            x[:, 2] = 0.75
            x[int(rng.integers(0, n_rows)), 2] = 5.0
        out.append(x.astype(F))
    return out


OFFSET_COLUMNS = (0,)  # of bounded_batches: |mean| / std = 1e5, where a cancelling variance loses everything

# max |state - fp64 rule| <= K * max |fp32 numpy rule - fp64 rule| per state vector and SHAPE (n_rows x dim), both maxima over the shape's
# BOUND_SEEDS draws x BOUND_UPDATES consecutive updates.  Why a maximum over draws: the state is fp32, so near mean 1e3 it sits on a 6e-5 grid
# while a batch moves the mean by ~std / sqrt(n) ~ 1e-3 .. 1e-4; every fp32 evaluation - the kernel's and numpy's - inherits delta with that
# grid's error and misses var by ~rate * delta * 3e-5 ~ 1e-8, EXCEPT in the draws where its mean happens to round the right way.  One draw of the
# yardstick is therefore 0 .. 2e-8 by luck (measured: 1.4e-10 beside 1.4e-8 for the same shape); sixteen are not.
# K is the next power of two at or above twice the largest ratio measured on the MI355X over ROWS x DIMS (profiles/obsnorm_accuracy.txt), never
# above 8.
K_STATE = 4.0  # largest measured ratio 1.624 (1 x 1, var)
K_CAP = 8.0


BOUND_SEEDS = 4
BOUND_UPDATES = 4


def bound_case(n_rows, dim, seed):
    """(batches, fp64 states, fp32 numpy states after each of the BOUND_UPDATES updates) of one draw of a shape"""
    batches = bounded_batches(n_rows, dim, BOUND_UPDATES, seed)
    ref, emu, refs, emus = fresh(dim, np.float64), fresh(dim, F), [], []
    for x in batches:
        ref, emu = rule(ref, x, np.float64), rule(emu, x, F)
        refs.append(ref)
        emus.append(emu)
    return batches, refs, emus


def vector_error(state, ref, k):
    return float(np.abs(np.asarray(state[k], np.float64).reshape(-1) - ref[k]).max())
