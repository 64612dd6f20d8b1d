"""The one copy of what the inference-MLP tests share (tests/test_policy.py, tests/test_policy_exact.py on the CPU,
tests/test_gpu_policy_exact.py on the GPU; the kernels: robot_lab_amd/csrc/rl_policy.hip):

  - the ROUTE TABLE: every way the host dispatch of rl_policy.hip reaches a kernel, as (environment, call) pairs, plus `kernel_for`,
    a restatement of that dispatch that names the kernel a (route, shapes, row count) lands on;
  - the EXACT families: signed selection networks (the output is an input column, bit for bit) and integer networks (every partial
    sum in any order is exact, checked in int64 before anything runs);
  - the fp32 REFERENCE and the bound E <= M * E32 on it, and the numpy EMULATION of the split-bf16 path with its faults (a product, a
    plane, a k block or a tile missing), which is what shows on the CPU that the bound has teeth.

`torch` is imported inside the functions: the module imports wherever its users do."""
import contextlib
import os

import numpy as np

from oracle.policy import mlp_forward

DEV = "cuda:0"

# ---- the dispatch of rl_policy.hip, restated ---------------------------------------------------------------------------------------
MT, LDS_MAX = 16, 160 * 1024
ENV_KEYS = ("RL_MLP_PRECISION", "RL_MLP_SPLIT_RT")  # read at every call
ONCE_KEYS = ("RL_MLP_PAIR_RT", "RL_MLP_PAIR_MODE", "RL_MLP_FUSED_WAVES")  # read once per process: the tests reach kernels by shape instead
# route -> (single | pair, environment of the call)
ROUTES = {
    "split16": ("single", {}),                                # rl_mlp_forward, default
    "split32": ("single", {"RL_MLP_SPLIT_RT": "2"}),
    "f32": ("single", {"RL_MLP_PRECISION": "f32"}),
    "small": ("single", {}),                                  # rl_mlp_forward_small
    "pair_split16": ("pair", {}),                             # rl_mlp_forward_pair, default
    "pair_split32": ("pair", {"RL_MLP_SPLIT_RT": "2"}),
    "pair_f32": ("pair", {"RL_MLP_PRECISION": "f32"}),
}
SINGLE_ROUTES = tuple(r for r, (k, _) in ROUTES.items() if k == "single")
PAIR_ROUTES = tuple(r for r, (k, _) in ROUTES.items() if k == "pair")
KERNELS = ("mlp_forward_kernel", "mlp_split_kernel", "mlp_split2_kernel", "mlp_forward_pair_kernel<1, 4>", "mlp_forward_pair_kernel<2, 8>",
           "mlp_fused_pair_kernel<16>")


def split_lds_bytes(dims):
    """rl_mlp_create / split_lds_bytes: layer l reads activation buffer l & 1, each as wide as its widest (32-padded) layer input"""
    cols = [0, 0]
    for l, k in enumerate(dims[:-1]):
        cols[l & 1] = max(cols[l & 1], (k + 31) // 32 * 32)
    return (cols[0] + cols[1]) * MT * 3 * 2


def kernel_for(route, n, dims, dims_b=None):
    """the kernel rl_mlp_forward / _small / _pair launches for `n` rows of the network(s) of these layer widths on `route`"""
    kind, env = ROUTES[route]
    f32, rt = env.get("RL_MLP_PRECISION") == "f32", int(env.get("RL_MLP_SPLIT_RT", "0"))
    if kind == "single":
        assert dims_b is None
        if route == "small" or f32 or split_lds_bytes(dims) > LDS_MAX:
            return "mlp_forward_kernel"
        two, big = 2 * split_lds_bytes(dims) <= LDS_MAX, n >= 8192
    else:
        la, lb = split_lds_bytes(dims), split_lds_bytes(dims_b)
        if f32 or len(dims) != len(dims_b) or la + lb > LDS_MAX:
            if len(dims) == len(dims_b) and n >= 3072:
                return "mlp_fused_pair_kernel<16>"
            return "mlp_forward_pair_kernel<2, 8>" if n >= 4096 else "mlp_forward_pair_kernel<1, 4>"
        two, big = 2 * max(la, lb) <= LDS_MAX, 2 * n >= 8192
    return "mlp_split2_kernel" if two and (rt == 2 or (rt != 1 and big)) else "mlp_split_kernel"


def pair_act_available(dims, dims_b, act_dim, f32=False):
    """rl_mlp_forward_pair_act: 0 (done in the launch) exactly when the pair runs a split-precision kernel"""
    return not f32 and len(dims) == len(dims_b) and split_lds_bytes(dims) + split_lds_bytes(dims_b) <= LDS_MAX and (act_dim + 3) // 4 * 32 <= 512


@contextlib.contextmanager
def route_env(route):
    for k in ONCE_KEYS:
        assert k not in os.environ, f"{k} is read once per process and would move every route"
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(ROUTES[route][1])
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_policy(ws, bs, act):
    from robot_lab_amd.policy import MlpPolicy

    return MlpPolicy(ws, bs, act, device=DEV)


def to_dev(x):
    import torch

    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def run_route(route, pol, x, other=None, other_x=None):
    """pol(x) - for a pair route (pol(x), other(other_x)) - through `route`, as numpy arrays (copies: the policies reuse their outputs)"""
    import torch

    xt = to_dev(x)
    with route_env(route):
        if ROUTES[route][0] == "single":
            if route == "small":
                out = torch.empty(xt.shape[0], pol.out_dim, device=DEV, dtype=torch.float32)
                pol.forward_into(xt, out.data_ptr(), small=True)
                return out.cpu().numpy()
            return pol(xt).cpu().numpy()
        ya, yb = pol.forward_pair(xt, other, to_dev(other_x))
        return ya.cpu().numpy(), yb.cpu().numpy()


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


# ---- exact family 1: signed selection networks -------------------------------------------------------------------------------------
def wide_inputs(rng, shape, positive):
    """full-significand fp32 numbers (23 random mantissa bits), magnitudes log-uniform in [2^-100, 2^100)"""
    u = rng.integers(0, 1 << 23, shape, dtype=np.uint32) | (rng.integers(27, 227, shape, dtype=np.uint32) << np.uint32(23))
    if not positive:
        u |= rng.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31)
    return u.view(np.float32)


def selection_rotations(dims):
    """how many rotations of `selection_net` put every input column of every layer on a path that ends in an output"""
    return -(-max(dims[:-1]) // min(dims[1:]))


def selection_net(dims, rot):
    """Every weight row holds a single +-1 (+1 in the layers a relu follows, alternating signs in the last), all biases 0: every layer copies
    or negates an input column.  Output n of rotation `rot` is path g = rot * m + n (m: the narrowest layer output), which runs through
    column g % dims[l] of layer l's input wherever that column is still free - a row that two paths want goes to the first, the later
    path then follows it.  Rows no path needs select column (row + rot) % width.  Returns (ws, bs, src, sgn, seen):
    y[:, n] = sgn[n] * x[:, src[n]] is the oracle, seen[l] the input columns of layer l that lie on a path to an output."""
    L, m = len(dims) - 1, min(dims[1:])
    sel = [(np.arange(dims[l + 1]) + rot) % dims[l] for l in range(L)]
    claim = {n: rot * m + n for n in range(dims[L])}  # row of the layer's output -> the path that owns it
    seen = [None] * L
    for l in range(L - 1, -1, -1):
        nxt = {}
        for row, g in claim.items():
            sel[l][row] = g % dims[l]
            nxt.setdefault(int(sel[l][row]), g)
        seen[l] = set(nxt)
        claim = nxt
    ws = []
    for l in range(L):
        w = np.zeros((dims[l + 1], dims[l]), dtype=np.float32)
        sign = np.where((np.arange(dims[l + 1]) + rot) % 2 == 1, -1.0, 1.0) if l == L - 1 else np.ones(dims[l + 1])
        w[np.arange(dims[l + 1]), sel[l]] = sign
        ws.append(w)
    bs = [np.zeros(d, dtype=np.float32) for d in dims[1:]]
    src = np.arange(dims[L])
    for l in range(L - 1, -1, -1):
        src = sel[l][src]
    sgn = np.where((np.arange(dims[L]) + rot) % 2 == 1, -1.0, 1.0).astype(np.float32)
    return ws, bs, src, sgn, seen


def selection_inputs(dims, rows, seed):
    """positive where a relu follows; both signs in single-layer networks (multi-layer ones see both signs through the last layer's -1 entries)"""
    return wide_inputs(np.random.default_rng(seed), (rows, dims[0]), positive=len(dims) > 2)


def selection_oracle(x, src, sgn):
    return x[:, src] * sgn  # a bit copy with the sign flipped where sgn is -1


# ---- exact family 2: integer networks ----------------------------------------------------------------------------------------------
SPAN = 1 << 24  # integers below it are exact in fp32


def _sig_bits(a):
    """most significant bits any entry of the integer array needs (bit length without its trailing zeros)"""
    a = np.abs(np.asarray(a, dtype=np.int64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return 0
    low = a & -a
    return int(np.floor(np.log2((a // low).max())) + 1)


def _sparse_units(rng, n_out, n_in, nnz):
    w = np.zeros((n_out, n_in), dtype=np.int64)
    for n in range(n_out):
        k = rng.choice(n_in, size=min(nnz, n_in), replace=False)
        w[n, k] = rng.choice([-1, 1], size=len(k))
    return w


def _wide_ints(rng, shape, max_bits):
    """signed integers whose bit length is uniform in 1..max_bits (so all three bf16 planes carry bits in the long ones)"""
    nb = rng.integers(1, max_bits + 1, shape)
    lo = np.left_shift(np.int64(1), nb - 1)
    return (lo + (rng.integers(0, 1 << 62, shape) % lo)) * rng.choice([-1, 1], shape)


def integer_net(dims, flavour, rows, seed, ex=0, ew=0):
    """An integer network and batch, everything times one power of two per tensor (inputs 2^ex, every weight matrix 2^ew, biases what
    their layer's sums carry).  Flavours: "wide_x" 24-bit inputs against weights in {-1, 0, 1} with at most four non-zeros per row;
    "wide_w" inputs of at most 3 bits against 20-bit weights in the first layer (sparse units behind it: its outputs are wide);
    "dense" dense inputs, weights and biases in [-3, 3].  ASSERTS in int64, before anything runs: in every layer one operand has at most 8
    significant bits (the three split products the kernel drops are then exactly zero) and sum_k |x_k| |w_k| + |b| < 2^24 units for
    every output of every row (every partial sum in any order is then exact in fp32).  Sparse rows that would break the span lose
    non-zeros until they fit.  Returns (x, ws, bs, want) in float32; want is the int64 forward (relu between the layers)."""
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    if flavour == "wide_x":
        X = _wide_ints(rng, (rows, dims[0]), 24)
    elif flavour == "wide_w":
        X = rng.integers(-7, 8, (rows, dims[0]))
    else:
        X = rng.integers(-3, 4, (rows, dims[0]))
    X = X.astype(np.int64)
    Ws, Bs, H = [], [], X
    for l in range(L):
        if flavour == "dense":
            W, b = rng.integers(-3, 4, (dims[l + 1], dims[l])).astype(np.int64), rng.integers(-3, 4, dims[l + 1]).astype(np.int64)
        else:
            if flavour == "wide_w" and l == 0:
                W = _sparse_units(rng, dims[1], dims[0], 6) * np.abs(_wide_ints(rng, (dims[1], dims[0]), 20))
            else:
                W = _sparse_units(rng, dims[l + 1], dims[l], 4)
            b = rng.integers(-5, 6, dims[l + 1]).astype(np.int64)
            Ha = np.abs(H)
            for n in range(dims[l + 1]):  # the span condition decides how many non-zeros a row keeps
                while True:
                    contrib = Ha * np.abs(W[n])  # [rows, K]
                    if contrib.sum(axis=1).max() + abs(b[n]) < SPAN:
                        break
                    W[n, np.argmax(contrib.max(axis=0))] = 0
        assert min(_sig_bits(H), _sig_bits(W)) <= 8, f"layer {l}: both operands are wider than 8 significant bits"
        span = np.abs(H) @ np.abs(W).T + np.abs(b)
        assert span.max() < SPAN, f"layer {l}: sum |x| |w| + |b| reaches {span.max()} >= 2^24"
        H = H @ W.T + b
        if l < L - 1:
            H = np.maximum(H, 0)
        Ws.append(W)
        Bs.append(b)
    scale = [ex + ew * (l + 1) for l in range(L)]  # exponent of layer l's sums

    def f32(a, e):
        out = np.ldexp(a.astype(np.float64), e).astype(np.float32)
        assert np.array_equal(np.ldexp(out.astype(np.float64), -e), a.astype(np.float64))  # representable as given
        return out

    return f32(X, ex), [f32(W, ew) for W in Ws], [f32(b, scale[l]) for l, b in enumerate(Bs)], f32(H, scale[-1])


# ---- the fp32 reference, the bound on it, and the emulation of the split path ------------------------------------------------------------
def _act64(v, act):
    v = v.astype(np.float64)
    if act == "elu":
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    return np.maximum(v, 0.0) if act == "relu" else np.tanh(v)


def fp32_reference(x, ws, bs, act):
    """a numpy float32 forward, layer by layer; the activation in float64, rounded to float32"""
    h = np.asarray(x, dtype=np.float32)
    for l, (w, b) in enumerate(zip(ws, bs)):
        h = h @ np.asarray(w, dtype=np.float32).T + np.asarray(b, dtype=np.float32)
        assert h.dtype == np.float32
        if l < len(ws) - 1:
            h = _act64(h, act).astype(np.float32)
    return h


def error_ratio(got, x, ws, bs, act, want=None):
    """(E, E32): max |got - oracle| and max |fp32_reference - oracle| over the batch"""
    want = mlp_forward(x, ws, bs, act) if want is None else want
    return float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(fp32_reference(x, ws, bs, act).astype(np.float64) - want).max())


# E <= M_BOUND * E32.  Where it comes from (profiles/mlp_accuracy.txt): on the MI355X the kernels measure at most 2.0 x E32 on either
# precision, every route and case (the one-row [48, 64] case of tests/test_policy.py; at most 1.1 x on 256 rows), so M >= 4 x that; the
# smallest emulated fault (both `lo` products missing in the last k block of the A1 actor) measures 35 x E32, so M <= that / 4.
M_BOUND = 8.0


def assert_fp32_bound(got, x, ws, bs, act, what="", want=None):
    e, e32 = error_ratio(got, x, ws, bs, act, want)
    print(f"[mlp bound] {what}: E = {e:.3e}, E32 = {e32:.3e}, E / E32 = {e / e32:.2f} (M = {M_BOUND:g})")
    assert e <= M_BOUND * e32, f"{what}: max |err| {e:.3e} is {e / e32:.1f} x the fp32 reference's {e32:.3e} (bound {M_BOUND:g} x)"
    return e / e32


def split3_np(v):
    """split3 of rl_policy.hip: three bf16 planes by truncation, hi + mid + lo == v; inf / nan stay in the leading plane"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    top = np.uint32(0xFFFF0000)
    h = (v.view(np.uint32) & top).view(np.float32)
    with np.errstate(invalid="ignore"):
        r = v - h
        m = (r.view(np.uint32) & top).view(np.float32)
        lo = ((r - m).view(np.uint32) & top).view(np.float32)
    fin = np.isfinite(v)
    return h, np.where(fin, m, np.float32(0)), np.where(fin, lo, np.float32(0))


PRODUCTS = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))  # (activation plane, weight plane): hi hi, hi mid, mid hi, mid mid, hi lo, lo hi
LO_PRODUCTS = ((0, 2), (2, 0))
FAULTS = tuple(("drop", p) for p in PRODUCTS) + (("lo_plane", None), ("lo_last_kblock", None), ("lo_tile", None))


def emulate_split(x, ws, bs, act, fault=None):
    """The split-bf16 path on the CPU: both operands as three truncated bf16 planes, the six plane products the kernel issues (summed in
    float64: exact enough to stand for the fp32 accumulators), ONE fp32 rounding per layer, the activation in float64 rounded to fp32.
    `fault` (in every layer): ("drop", (a, b)) that product missing; ("lo_plane", None) both products of a `lo` plane missing;
    ("lo_last_kblock", None) those two missing in the last 32-deep k block only; ("lo_tile", None) missing in output columns 0..15 only."""
    kind, arg = fault if fault else (None, None)
    h = np.asarray(x, dtype=np.float32)
    for l, (w, b) in enumerate(zip(ws, bs)):
        xp = [p.astype(np.float64) for p in split3_np(h)]
        wp = [p.astype(np.float64) for p in split3_np(w)]
        K = w.shape[1]
        acc = np.zeros((h.shape[0], w.shape[0]))
        for a, c in PRODUCTS:
            if (kind == "drop" and (a, c) == arg) or (kind == "lo_plane" and (a, c) in LO_PRODUCTS):
                continue
            part = xp[a] @ wp[c].T
            if (a, c) in LO_PRODUCTS:
                if kind == "lo_last_kblock":
                    k0 = (K - 1) // 32 * 32
                    part -= xp[a][:, k0:] @ wp[c][:, k0:].T
                elif kind == "lo_tile":
                    part[:, :16] = 0.0
            acc += part
        h = (acc + np.asarray(b, dtype=np.float64)).astype(np.float32)
        if l < len(ws) - 1:
            h = _act64(h, act).astype(np.float32)
    return h


def random_net(dims, seed):
    """tests/test_policy.py `_net`: weights N(0, 1 / fan-in), biases N(0, 0.01)"""
    rng = np.random.default_rng(seed)
    ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    bs = [(0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32) for i in range(len(dims) - 1)]
    return ws, bs


# the cases of the bound: (widths, activation); 256 rows each so that the maxima are stable
BOUND_CASES = [([45, 512, 256, 128, 12], "elu"), ([235, 512, 256, 128, 1], "elu"), ([7, 33, 5], "tanh"), ([48, 64], "relu")]
BOUND_ROWS = 256


def bound_case(dims, act):
    ws, bs = random_net(dims, 3)
    x = np.random.default_rng(4).uniform(-2, 2, (BOUND_ROWS, dims[0])).astype(np.float32)
    return x, ws, bs


# ---- case tables (tests/test_policy_exact.py checks on the CPU what they cover) -----------------------------------------------------------
# selection networks: (layer widths, rows); layer counts 1, 2, 4, 5, 8
SELECTION_CASES = [
    ([1, 1], 1), ([31, 12], 15), ([33, 1], 16), ([512, 29], 37),
    ([32, 16, 12], 32), ([480, 512, 29], 17), ([65, 129, 12], 31), ([31, 1, 12], 33),
    ([45, 512, 128, 127, 29], 32), ([235, 400, 33, 17, 29], 37),
    ([33, 15, 16, 17, 127, 12], 15),
    ([65, 128, 129, 33, 17, 16, 15, 33, 29], 33), ([512, 512, 400, 128, 129, 127, 33, 16, 12], 17),
]
_A4, _C4 = [45, 512, 128, 127, 12], [235, 400, 33, 17, 1]
_A2 = [45, 128, 12]
_G1A, _G1C = [480, 512, 256, 128, 29], [310, 512, 256, 128, 1]  # the G1 networks on an observation history of 5
_A8, _C8 = [65, 128, 129, 33, 17, 16, 15, 33, 29], [512, 512, 400, 128, 129, 127, 33, 16, 12]
_P14, _P28, _FUSED = "mlp_forward_pair_kernel<1, 4>", "mlp_forward_pair_kernel<2, 8>", "mlp_fused_pair_kernel<16>"
# pairs: (actor widths, critic widths, rows, {route: the kernel it must land on})
PAIR_CASES = [
    (_A4, _C4, 37, {"pair_split16": "mlp_split_kernel", "pair_split32": "mlp_split2_kernel", "pair_f32": _P14}),
    (_A4, _C4, 4099, {"pair_split16": "mlp_split2_kernel", "pair_f32": _FUSED}),            # the big routes of an equal-depth pair
    (_A2, _C4, 37, {"pair_split16": _P14, "pair_f32": _P14}),                                # unequal depth: the f32 kernels, whatever the precision
    (_A2, _C4, 4099, {"pair_split16": _P28, "pair_f32": _P28}),
    (_G1A, _G1C, 37, {"pair_split16": _P14, "pair_split32": _P14}),                          # LDS fallback of a pair
    (_A8, _C8, 33, {"pair_split16": "mlp_split_kernel", "pair_split32": "mlp_split_kernel", "pair_f32": _P14}),  # eight layers; no room for 32 rows
]
# integer networks: (layer widths, flavour, rows, exponent of the inputs, exponent of every weight matrix)
INTEGER_CASES = [
    (_A4, "wide_x", 37, -9, 2), (_C4, "wide_x", 33, 5, -1), ([33, 15, 16, 17, 127, 12], "wide_x", 17, 0, 0), (_A8, "wide_x", 31, -3, 1),
    ([512, 29], "wide_x", 16, 40, -20),
    (_A4, "wide_w", 37, 3, -12), ([480, 512, 29], "wide_w", 15, 0, 0), ([31, 12], "wide_w", 1, -2, 7), (_C4, "wide_w", 32, 0, -3),
    ([33, 17, 130, 5], "dense", 37, 0, 0), ([45, 64, 12], "dense", 33, -4, 2), ([235, 512, 1], "dense", 17, 1, 1),
]
