"""The inference-MLP tests' own teeth, on the CPU (tests/policy_helpers.py; the GPU side is tests/test_gpu_policy_exact.py):
the emulated split-bf16 path passes the fp32-referenced bound and every emulated fault fails it, split3 is exact, the exact families'
oracles and conditions hold, and the case tables reach every kernel of the dispatch."""
import numpy as np
import pytest

import policy_helpers as ph
from oracle.policy import mlp_forward
from policy_helpers import INTEGER_CASES, PAIR_CASES, SELECTION_CASES


@pytest.fixture(scope="module", params=range(len(ph.BOUND_CASES)), ids=[f"{d}-{a}" for d, a in ph.BOUND_CASES])
def bound_case(request):
    dims, act = ph.BOUND_CASES[request.param]
    x, ws, bs = ph.bound_case(dims, act)
    want = mlp_forward(x, ws, bs, act)
    e32 = float(np.abs(ph.fp32_reference(x, ws, bs, act).astype(np.float64) - want).max())
    return dims, act, x, ws, bs, want, e32


def test_faithful_emulation_passes_the_bound(bound_case):
    dims, act, x, ws, bs, want, e32 = bound_case
    ratio = ph.assert_fp32_bound(ph.emulate_split(x, ws, bs, act), x, ws, bs, act, f"emulated split path {dims} {act}", want)
    assert 4.0 * ratio <= ph.M_BOUND  # the margin the bound keeps over a healthy path


@pytest.mark.parametrize("fault", ph.FAULTS, ids=[f"{k}{'' if a is None else '-%d%d' % a}" for k, a in ph.FAULTS])
def test_every_emulated_fault_fails_the_bound(bound_case, fault):
    """each of the six products removed in turn, the lo plane removed, both lo products removed in the last k block only, one 16-column
    output tile without its lo products: every one is at least 4 x over the bound, on every case"""
    dims, act, x, ws, bs, want, e32 = bound_case
    e = float(np.abs(ph.emulate_split(x, ws, bs, act, fault).astype(np.float64) - want).max())
    print(f"[mlp teeth] {dims} {act} {fault}: E / E32 = {e / e32:.1f}")
    assert e > ph.M_BOUND * e32
    assert e >= 4.0 * ph.M_BOUND * e32
    with pytest.raises(AssertionError):
        ph.assert_fp32_bound(ph.emulate_split(x, ws, bs, act, fault), x, ws, bs, act, "faulty", want)


def test_split3_sums_back_exactly():
    """hi + mid + lo == x for 10^5 random bit patterns of normal floats at or above 2^-100, each plane a bf16 number, (lo + mid) + hi in
    fp32 included (the order the kernel's accumulators meet in)"""
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1 << 23, 100000, dtype=np.uint32) | (rng.integers(27, 255, 100000, dtype=np.uint32) << np.uint32(23)) | (rng.integers(0, 2, 100000, dtype=np.uint32) << np.uint32(31))
    x = u.view(np.float32)
    assert np.isfinite(x).all() and np.abs(x).min() >= 2.0 ** -100
    h, m, lo = ph.split3_np(x)
    for p in (h, m, lo):
        assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))
    ph.assert_bits_equal((lo + m) + h, x, "(lo + mid) + hi")
    # inf / nan: the leading plane only
    h, m, lo = ph.split3_np(np.array([np.inf, -np.inf, np.nan], dtype=np.float32))
    assert np.isinf(h[:2]).all() and np.isnan(h[2]) and not m.any() and not lo.any()


@pytest.mark.parametrize("dims,rows", SELECTION_CASES, ids=str)
def test_selection_rotations_cover_every_column(dims, rows):
    """over its rotations every input column of every layer lies on a path to an output, every row holds a single +-1, and the
    fp64 oracle of the network is the bit copy the GPU test compares with"""
    L = len(dims) - 1
    seen = [set() for _ in range(L)]
    x = ph.selection_inputs(dims, rows, 1)
    assert np.abs(x).min() >= 2.0 ** -100 and np.abs(x).max() < 2.0 ** 100 and (len(dims) == 2) == bool((x < 0).any())
    negated = False
    for rot in range(ph.selection_rotations(dims)):
        ws, bs, src, sgn, s = ph.selection_net(dims, rot)
        for l in range(L):
            seen[l] |= s[l]
            assert ((ws[l] != 0).sum(axis=1) == 1).all() and set(np.unique(ws[l])) <= {-1.0, 0.0, 1.0} and not bs[l].any()
            assert l == L - 1 or (ws[l] >= 0).all()
        negated |= bool((sgn < 0).any())
        if rot in (0, 1):
            ph.assert_bits_equal(mlp_forward(x, ws, bs, "relu").astype(np.float32), ph.selection_oracle(x, src, sgn), f"rotation {rot}")
    assert negated or dims[-1] == 1 and ph.selection_rotations(dims) == 1
    for l in range(L):
        assert seen[l] == set(range(dims[l])), f"layer {l}: columns {sorted(set(range(dims[l])) - seen[l])[:8]} never selected"


def test_selection_cases_span_the_issue_lists():
    firsts, hidden, outs, depths, rows = set(), set(), set(), set(), set()
    for dims, r in SELECTION_CASES:
        firsts.add(dims[0]); hidden.update(dims[1:-1]); outs.add(dims[-1]); depths.add(len(dims) - 1); rows.add(r)
    assert firsts == {1, 31, 32, 33, 45, 65, 235, 480, 512}
    assert hidden == {1, 15, 16, 17, 33, 127, 128, 129, 400, 512}
    assert outs == {1, 12, 29} and depths == {1, 2, 4, 5, 8} and rows == {1, 15, 16, 17, 31, 32, 33, 37}


@pytest.mark.parametrize("dims,flavour,rows,ex,ew", INTEGER_CASES, ids=str)
def test_integer_nets_meet_their_conditions(dims, flavour, rows, ex, ew):
    """integer_net asserts the 8-bit and the span condition itself; here: its int64 forward is what the fp64 oracle computes, the planes
    it promises carry bits, and the numpy fp32 forward and the split emulation already reproduce it bit for bit"""
    x, ws, bs, want = ph.integer_net(dims, flavour, rows, 2, ex, ew)
    ph.assert_bits_equal(mlp_forward(x, ws, bs, "relu").astype(np.float32), want, "fp64 oracle")
    ph.assert_bits_equal(ph.fp32_reference(x, ws, bs, "relu"), want, "numpy fp32")
    ph.assert_bits_equal(ph.emulate_split(x, ws, bs, "relu"), want, "split emulation")
    if flavour == "wide_x":
        assert ph.split3_np(x)[2].any()  # the inputs' lo plane is in use
    if flavour == "wide_w":
        assert ph.split3_np(ws[0])[2].any() and np.abs(x).max() <= np.ldexp(7.0, ex)
    assert want.any()


def test_case_tables_reach_every_kernel():
    """the dispatch restated in policy_helpers.kernel_for, applied to the GPU test's case tables: every kernel of rl_policy.hip is launched,
    the 32-row request of a 480 / 512-wide first layer lands on the 16-row kernel, the G1 history pair on the f32 kernels"""
    reached = set()
    for dims, rows in SELECTION_CASES:
        for route in ph.SINGLE_ROUTES:
            reached.add(ph.kernel_for(route, rows, dims))
    for da, dc, rows, routes in PAIR_CASES:
        for route, want in routes.items():
            k = ph.kernel_for(route, rows, da, dc)
            assert k == want, (da, dc, rows, route, k)
            reached.add(k)
    assert reached == set(ph.KERNELS)
    for first in (480, 512):
        assert ph.split_lds_bytes([first, 512, 29]) <= ph.LDS_MAX < 2 * ph.split_lds_bytes([first, 512, 29])
        assert ph.kernel_for("split32", 17, [first, 512, 29]) == "mlp_split_kernel"
    g1a, g1c = [480, 512, 256, 128, 29], [310, 512, 256, 128, 1]
    assert ph.split_lds_bytes(g1a) <= ph.LDS_MAX < ph.split_lds_bytes(g1a) + ph.split_lds_bytes(g1c)
    assert ph.kernel_for("pair_split16", 37, g1a, g1c) == "mlp_forward_pair_kernel<1, 4>" and not ph.pair_act_available(g1a, g1c, 29)
