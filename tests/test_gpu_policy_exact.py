"""Inference MLP (robot_lab_amd/csrc/rl_policy.hip) on every kernel route: exact families with no tolerance, the bound tied to the fp32
reference, the activations on their own, non-finite rows, and the act epilogue off the beaten shape.  Helpers, case tables and the
reasoning behind each family: tests/policy_helpers.py; what the case tables cover and the bound's teeth: tests/test_policy_exact.py."""
import ctypes as C

import numpy as np
import pytest

import policy_helpers as ph
from oracle.policy import mlp_forward

pytestmark = pytest.mark.gpu

BIG = 4099  # rows of the routes that only large batches reach: 256 full 16-row tiles and a ragged one


def _ids(cases):
    return [str(c) for c in cases]


# ---- B.1 signed selection networks -------------------------------------------------------------------------------------------------------
def _set(pol, ws, bs, device_side, keep):
    """new weights in place: rl_mlp_set_weights, or rl_mlp_set_weights_device from device copies (kept alive in `keep`)"""
    import torch

    if device_side:
        keep[:] = [torch.from_numpy(a).to(ph.DEV) for a in ws + bs]
        pol.set_weights_device(keep[:len(ws)], keep[len(ws):])
    else:
        pol.set_weights(ws, bs)


@pytest.mark.parametrize("dims,rows", ph.SELECTION_CASES, ids=_ids(ph.SELECTION_CASES))
def test_selection_networks_copy_their_inputs_bit_for_bit(dims, rows):
    """every layer copies (the last one: or negates) an input column: the output is the selected input's bits on every single-network route -
    on the split path (lo + mid) + hi rebuilds x in every layer.  Over the rotations every input column of every layer is on a path to an
    output (tests/test_policy_exact.py); rotation 1 arrives through rl_mlp_set_weights_device, the later ones through rl_mlp_set_weights."""
    x = ph.selection_inputs(dims, rows, 21)
    xt, pol, keep = ph.to_dev(x), None, []
    for rot in range(ph.selection_rotations(dims)):
        ws, bs, src, sgn, _ = ph.selection_net(dims, rot)
        if pol is None:
            pol = ph.make_policy(ws, bs, "relu")
        else:
            _set(pol, ws, bs, rot == 1, keep)
        want = ph.selection_oracle(x, src, sgn)
        for route in ph.SINGLE_ROUTES:
            ph.assert_bits_equal(ph.run_route(route, pol, xt), want, f"{dims} x {rows}, rotation {rot}, {route} ({ph.kernel_for(route, rows, dims)})")
    pol.close()


@pytest.mark.parametrize("da,dc,rows,routes", ph.PAIR_CASES, ids=_ids([c[:3] for c in ph.PAIR_CASES]))
def test_selection_pairs_copy_their_inputs_bit_for_bit(da, dc, rows, routes):
    """the same through rl_mlp_forward_pair: both split pair kernels, the three f32 pair kernels (unequal depths reach <1, 4> and, from 4096
    rows on, <2, 8>; equal depths the fused kernel), eight layers, and the pair whose planes do not fit the LDS (the f32 kernels answer)"""
    xa, xc = ph.selection_inputs(da, rows, 22), ph.selection_inputs(dc, rows, 23)
    xat, xct, pa, pc, keep_a, keep_c = ph.to_dev(xa), ph.to_dev(xc), None, None, [], []
    ra, rc = ph.selection_rotations(da), ph.selection_rotations(dc)
    spread = [0, 1] if rows >= BIG else [0, 1, 2, 3]  # (full coverage is the single-network test's; here: the pair kernels' own plumbing)
    for i in spread:
        rot_a, rot_c = i * max(1, ra // 4) % ra, i * max(1, rc // 4) % rc
        na, nc = ph.selection_net(da, rot_a), ph.selection_net(dc, rot_c)
        if pa is None:
            pa, pc = ph.make_policy(na[0], na[1], "relu"), ph.make_policy(nc[0], nc[1], "relu")
        else:
            _set(pa, na[0], na[1], i == 1, keep_a)
            _set(pc, nc[0], nc[1], i == 1, keep_c)
        for route in routes:
            ya, yc = ph.run_route(route, pa, xat, pc, xct)
            what = f"{da} + {dc} x {rows}, rotations {rot_a} / {rot_c}, {route} ({ph.kernel_for(route, rows, da, dc)})"
            ph.assert_bits_equal(ya, ph.selection_oracle(xa, na[2], na[3]), "actor of " + what)
            ph.assert_bits_equal(yc, ph.selection_oracle(xc, nc[2], nc[3]), "critic of " + what)
    pa.close()
    pc.close()


# ---- B.2 integer networks ------------------------------------------------------------------------------------------------------------------
def _tiled(x, want, rows):
    """`rows` rows by repeating the batch (the conditions integer_net asserted hold row by row)"""
    idx = np.arange(rows) % x.shape[0]
    return np.ascontiguousarray(x[idx]), np.ascontiguousarray(want[idx])


@pytest.mark.parametrize("dims,flavour,rows,ex,ew", ph.INTEGER_CASES, ids=_ids(ph.INTEGER_CASES))
def test_integer_networks_equal_the_int64_forward(dims, flavour, rows, ex, ew):
    """integers times a power of two, one operand of every layer at most 8 significant bits wide, every sum of magnitudes below 2^24 units
    (asserted in int64 by the helper): every partial sum in any order is exact and the three split products the kernel leaves out are zero,
    so every route must give the int64 forward bit for bit.  A case that passes on f32 and fails on a split route would refute the claim
    that every bf16 x bf16 product is exact in the MFMA's accumulator."""
    x, ws, bs, want = ph.integer_net(dims, flavour, rows, 2, ex, ew)
    pol, xt = ph.make_policy(ws, bs, "relu"), ph.to_dev(x)
    for route in ph.SINGLE_ROUTES:
        ph.assert_bits_equal(ph.run_route(route, pol, xt), want, f"{flavour} {dims} x {rows}, {route} ({ph.kernel_for(route, rows, dims)})")
    pol.close()


_A4, _C4, _A2 = [45, 512, 128, 127, 12], [235, 400, 33, 17, 1], [45, 64, 12]
INTEGER_PAIRS = [  # (actor, its flavour, critic, its flavour, rows, routes)
    (_A4, "wide_x", _C4, "wide_w", 37, ("pair_split16", "pair_split32", "pair_f32")),
    (_A4, "wide_w", _C4, "wide_x", BIG, ("pair_split16", "pair_f32")),  # 32-row split kernel; fused f32 kernel
    (_A2, "dense", _C4, "wide_x", 37, ("pair_split16", "pair_f32")),    # unequal depth: <1, 4>
    (_A2, "dense", _C4, "wide_w", BIG, ("pair_split16",)),              # unequal depth: <2, 8>
]


@pytest.mark.parametrize("da,fa,dc,fc,rows,routes", INTEGER_PAIRS, ids=_ids([(c[1], c[3], c[4]) for c in INTEGER_PAIRS]))
def test_integer_pairs_equal_the_int64_forward(da, fa, dc, fc, rows, routes):
    xa, wa, ba, want_a = ph.integer_net(da, fa, 37, 5, -2, 1)
    xc, wc, bc, want_c = ph.integer_net(dc, fc, 37, 6, 1, -1)
    (xa, want_a), (xc, want_c) = _tiled(xa, want_a, rows), _tiled(xc, want_c, rows)
    pa, pc, xat, xct = ph.make_policy(wa, ba, "relu"), ph.make_policy(wc, bc, "relu"), ph.to_dev(xa), ph.to_dev(xc)
    for route in routes:
        ya, yc = ph.run_route(route, pa, xat, pc, xct)
        what = f"{fa} {da} + {fc} {dc} x {rows}, {route} ({ph.kernel_for(route, rows, da, dc)})"
        ph.assert_bits_equal(ya, want_a, "actor of " + what)
        ph.assert_bits_equal(yc, want_c, "critic of " + what)
    pa.close()
    pc.close()


# ---- C. the bound tied to the fp32 reference -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bound_refs():
    """per case: inputs, network, fp64 oracle - computed once"""
    out = {}
    for dims, act in ph.BOUND_CASES:
        x, ws, bs = ph.bound_case(dims, act)
        out[(tuple(dims), act)] = (x, ws, bs, mlp_forward(x, ws, bs, act))
    return out


@pytest.mark.parametrize("dims,act", ph.BOUND_CASES, ids=_ids(ph.BOUND_CASES))
def test_random_networks_stay_within_the_fp32_reference_bound(dims, act, bound_refs):
    """max |kernel - oracle| <= M x max |numpy fp32 forward - oracle| on every single-network route, both precisions (M, what the kernels
    measure and what the emulated faults measure: policy_helpers.M_BOUND, profiles/mlp_accuracy.txt)"""
    x, ws, bs, want = bound_refs[(tuple(dims), act)]
    pol, xt = ph.make_policy(ws, bs, act), ph.to_dev(x)
    for route in ph.SINGLE_ROUTES:
        ph.assert_fp32_bound(ph.run_route(route, pol, xt), x, ws, bs, act, f"{dims} {act} x {ph.BOUND_ROWS}, {route}", want)
    pol.close()


@pytest.mark.parametrize("route", ph.PAIR_ROUTES)
def test_the_a1_pair_stays_within_the_fp32_reference_bound(route, bound_refs):
    (da, aa), (dc, ac) = ph.BOUND_CASES[0], ph.BOUND_CASES[1]
    xa, wa, ba, want_a = bound_refs[(tuple(da), aa)]
    xc, wc, bc, want_c = bound_refs[(tuple(dc), ac)]
    pa, pc = ph.make_policy(wa, ba, aa), ph.make_policy(wc, bc, ac)
    ya, yc = ph.run_route(route, pa, xa, pc, xc)
    ph.assert_fp32_bound(ya, xa, wa, ba, aa, f"{da} {aa} x {ph.BOUND_ROWS}, {route}", want_a)
    ph.assert_fp32_bound(yc, xc, wc, bc, ac, f"{dc} {ac} x {ph.BOUND_ROWS}, {route}", want_c)
    pa.close()
    pc.close()


# ---- D. the activations on their own -------------------------------------------------------------------------------------------------------
ACT_WIDTH, ACT_ROWS = 129, 37


def _activation_sweep():
    """+-2^k for k = -30..6, +-100, and a dense grid on [-20, 20] filling the rest of a 37 x 129 batch"""
    pows = np.concatenate([s * np.ldexp(1.0, np.arange(-30, 7)) for s in (1.0, -1.0)])
    special = np.concatenate([pows, [100.0, -100.0]])
    grid = np.linspace(-20.0, 20.0, ACT_WIDTH * ACT_ROWS - special.size)
    return np.concatenate([special, grid]).astype(np.float32).reshape(ACT_ROWS, ACT_WIDTH)


@pytest.mark.parametrize("act", ["relu", "elu", "tanh"])
def test_activations_element_by_element(act):
    """a two-layer identity network makes y = act(x): relu exact; ELU exact for x > 0 and within 2^-22 of expm1 for x <= 0 (three roundings of
    at most one ulp at unit scale: the log2(e) product, v_exp_f32, the subtraction); tanh within 2^-22 - on the split and the f32 routes"""
    x = _activation_sweep()
    eye = np.eye(ACT_WIDTH, dtype=np.float32)
    zero = np.zeros(ACT_WIDTH, dtype=np.float32)
    pol, xt = ph.make_policy([eye, eye], [zero, zero], act), ph.to_dev(x)
    x64 = x.astype(np.float64)
    for route in ph.SINGLE_ROUTES:
        y = ph.run_route(route, pol, xt)
        what = f"{act}, {route}"
        if act == "relu":
            ph.assert_bits_equal(y, np.maximum(x, np.float32(0.0)), what)
            continue
        want = np.tanh(x64) if act == "tanh" else np.where(x64 > 0, x64, np.expm1(np.minimum(x64, 0.0)))
        err = np.abs(y.astype(np.float64) - want)
        i = np.unravel_index(np.argmax(err), err.shape)
        print(f"[mlp activation] {what}: max |err| = {err.max():.3e} = 2^{np.log2(max(err.max(), 1e-300)):.2f} at x = {x[i]!r}")
        if act == "elu":
            ph.assert_bits_equal(y[x > 0], x[x > 0], what + ", x > 0")
        assert err.max() <= 2.0 ** -22, f"{what}: |err| {err.max():.3e} at x = {x[i]!r} exceeds 2^-22 = {2.0 ** -22:.3e}"
    pol.close()


# ---- E. non-finite rows --------------------------------------------------------------------------------------------------------------------
NF_ACTOR, NF_CRITIC, NF_ROWS = [45, 64, 33, 12], [33, 129, 17, 1], 37
POISON = [("nan", 5, np.nan), ("inf", 20, np.inf)]


def _check_poisoned(got, clean, oracle, row, value, what):
    rest = np.arange(got.shape[0]) != row
    ph.assert_bits_equal(got[rest], clean[rest], what + ": rows beside the poisoned one")
    bad = ~np.isfinite(oracle[row])
    assert not np.isfinite(got[row][bad]).any(), f"{what}: row {row} is finite ({got[row]}) where the oracle is not ({oracle[row]})"
    if np.isnan(value):
        assert bad.all() and np.isnan(got[row]).all(), f"{what}: a NaN input must give a NaN row, got {got[row]}"


@pytest.mark.parametrize("act", ["elu", "relu", "tanh"])
def test_a_non_finite_row_stays_in_its_row_and_stays_non_finite(act):
    """row 5 holding a NaN, then row 20 holding +inf: every other row - the ones sharing a tile with it included - keeps the bits of the clean
    run, and the poisoned row is non-finite wherever the oracle's is (NaN throughout for a NaN input), on every single and pair route"""
    (wa, ba), (wc, bc) = ph.random_net(NF_ACTOR, 31), ph.random_net(NF_CRITIC, 32)
    rng = np.random.default_rng(33)
    xa, xc = rng.uniform(-2, 2, (NF_ROWS, NF_ACTOR[0])).astype(np.float32), rng.uniform(-2, 2, (NF_ROWS, NF_CRITIC[0])).astype(np.float32)
    pa, pc = ph.make_policy(wa, ba, act), ph.make_policy(wc, bc, act)
    clean = {r: ph.run_route(r, pa, xa) for r in ph.SINGLE_ROUTES}
    clean.update({r: ph.run_route(r, pa, xa, pc, xc) for r in ph.PAIR_ROUTES})
    for name, row, value in POISON:
        pxa, pxc = xa.copy(), xc.copy()
        pxa[row, 7] = value
        pxc[row, 3] = value
        with np.errstate(invalid="ignore"):
            oa, oc = mlp_forward(pxa, wa, ba, act), mlp_forward(pxc, wc, bc, act)
        for r in ph.SINGLE_ROUTES:
            _check_poisoned(ph.run_route(r, pa, pxa), clean[r], oa, row, value, f"{act}, {name} in row {row}, {r}")
        for r in ph.PAIR_ROUTES:
            ya, yc = ph.run_route(r, pa, pxa, pc, pxc)
            _check_poisoned(ya, clean[r][0], oa, row, value, f"{act}, {name} in row {row}, actor of {r}")
            _check_poisoned(yc, clean[r][1], oc, row, value, f"{act}, {name} in row {row}, critic of {r}")
    pa.close()
    pc.close()


def test_the_lds_fallbacks_answer_and_report():
    """a 480- or 512-wide first layer leaves no room for the 32-row kernel's planes: a forced 32-row call is answered by the 16-row kernel
    with the default call's bits; the G1 pair on an observation history of 5 (480 + 310 columns) does not fit the split pair kernels at all:
    the f32 kernels answer (the bits of the f32 single launches) and rl_mlp_forward_pair_act reports 1"""
    import torch

    from robot_lab_amd.rollout import ActEpilogue

    rows = 37
    rng = np.random.default_rng(41)
    for first in (480, 512):
        dims = [first, 512, 256, 128, 29]
        assert ph.kernel_for("split32", rows, dims) == "mlp_split_kernel"
        ws, bs = ph.random_net(dims, first)
        x = rng.uniform(-2, 2, (rows, first)).astype(np.float32)
        pol = ph.make_policy(ws, bs, "elu")
        y16, y32 = ph.run_route("split16", pol, x), ph.run_route("split32", pol, x)
        ph.assert_bits_equal(y32, y16, f"first width {first}: forced 32-row call")
        ph.assert_fp32_bound(y32, x, ws, bs, "elu", f"{dims} elu x {rows}, split32 -> 16-row kernel")
        pol.close()
    da, dc = [480, 512, 256, 128, 29], [310, 512, 256, 128, 1]
    (wa, ba), (wc, bc) = ph.random_net(da, 42), ph.random_net(dc, 43)
    xa, xc = rng.uniform(-2, 2, (rows, da[0])).astype(np.float32), rng.uniform(-2, 2, (rows, dc[0])).astype(np.float32)
    pa, pc = ph.make_policy(wa, ba, "elu"), ph.make_policy(wc, bc, "elu")
    fa, fc = ph.run_route("f32", pa, xa), ph.run_route("f32", pc, xc)
    for route in ("pair_split16", "pair_split32"):
        assert ph.kernel_for(route, rows, da, dc) == "mlp_forward_pair_kernel<1, 4>"
        ya, yc = ph.run_route(route, pa, xa, pc, xc)
        ph.assert_bits_equal(ya, fa, f"G1 history pair, actor, {route}")
        ph.assert_bits_equal(yc, fc, f"G1 history pair, critic, {route}")
    # the act launch is not available: 1, and nothing written
    assert not ph.pair_act_available(da, dc, 29)
    sent = torch.full((rows, 480), 7.5, device=ph.DEV)  # (as large as the largest buffer the epilogue names)
    v = torch.full((rows,), 7.5, device=ph.DEV)
    std, ctr = torch.ones(29, device=ph.DEV), torch.zeros(4, dtype=torch.int32, device=ph.DEV)
    p = sent.data_ptr()
    ep = ActEpilogue(actions_out=p, s_obs=p, s_critic_obs=p, s_actions=p, s_mu=p, s_sigma=p, s_logp=v.data_ptr(), s_values=v.data_ptr(), std=std.data_ptr(),
                     counter_base=ctr.data_ptr(), seed=1, counter=0, num_envs=rows, obs_dim=480, critic_dim=310, act_dim=29, clip=-1.0)
    with ph.route_env("pair_split16"):
        assert pa.forward_pair_act(C.c_void_p(ph.to_dev(xa).data_ptr()), pc, C.c_void_p(ph.to_dev(xc).data_ptr()), ep) == 1
    torch.cuda.synchronize()
    assert bool((sent == 7.5).all()) and bool((v == 7.5).all())
    pa.close()
    pc.close()


# ---- F. the act epilogue off the beaten shape --------------------------------------------------------------------------------------------------
ACT_CASES = [(37, 45, 235, 12), (37, 96, 310, 29), (33, 5, 7, 1), (1, 45, 235, 12)]  # (N, obs, critic obs, A)
SENTINEL = -123.25
SLOT_NAMES = ("observations", "privileged_observations", "actions", "mu", "sigma", "actions_log_prob", "values")


@pytest.mark.parametrize("clip", [None, 0.8])
@pytest.mark.parametrize("rt", ["1", "2"])
@pytest.mark.parametrize("N,od,cd,A", ACT_CASES, ids=_ids(ACT_CASES))
def test_act_epilogue_equals_pair_then_act_kernel(N, od, cd, A, rt, clip, monkeypatch):
    """rl_mlp_forward_pair_act against rl_mlp_forward_pair + rl_rollout_act on a twin storage, synthetic networks, no env: a ragged last tile,
    an action width that is no multiple of the 4-wide Philox block (29), a single action, a single row; both split pair kernels; with and
    without the clamp.  Everything the step writes is bit-equal, and nothing is written behind row N of any buffer."""
    import torch

    from robot_lab_amd.rollout import ActEpilogue, RolloutStorage

    monkeypatch.delenv("RL_MLP_PRECISION", raising=False)
    monkeypatch.setenv("RL_MLP_SPLIT_RT", rt)
    da, dc = [od, 64, 33, A], [cd, 128, 17, 1]
    assert ph.pair_act_available(da, dc, A)
    assert ph.kernel_for("pair_split32" if rt == "2" else "pair_split16", N, da, dc) == ("mlp_split2_kernel" if rt == "2" else "mlp_split_kernel")
    (wa, ba), (wc, bc) = ph.random_net(da, 51), ph.random_net(dc, 52)
    actor, critic = ph.make_policy(wa, ba, "elu"), ph.make_policy(wc, bc, "elu")
    rng = np.random.default_rng(53)
    xo, xc = ph.to_dev(rng.uniform(-2, 2, (N, od)).astype(np.float32)), ph.to_dev(rng.uniform(-2, 2, (N, cd)).astype(np.float32))
    std = ph.to_dev(rng.uniform(0.3, 1.2, A).astype(np.float32))
    pad = 5  # sentinel rows behind every output

    def side(fused):
        st = RolloutStorage(N, 2, od, cd, A, seed=9, device=ph.DEV)  # slot 1 is what lies behind row N of slot 0
        for name in SLOT_NAMES:
            getattr(st, name).fill_(SENTINEL)
        act_out = torch.full((N + pad, A), SENTINEL, device=ph.DEV)
        mean = torch.full((N + pad, A), SENTINEL, device=ph.DEV)
        st._actions, actor._out = act_out[:N], mean[:N]
        if fused:
            ep = ActEpilogue()
            assert st.lib.rl_rollout_act_epilogue(st.handle, C.c_void_p(std.data_ptr()), C.c_void_p(act_out.data_ptr()), -1.0 if clip is None else clip, C.byref(ep)) == 0
            assert actor.forward_pair_act(C.c_void_p(xo.data_ptr()), critic, C.c_void_p(xc.data_ptr()), ep) == 0  # really in the launch
            assert st.lib.rl_rollout_act_done(st.handle) == 0
            actions = act_out[:N].clone()
        else:
            mu, values = actor.forward_pair(xo, critic, xc)
            assert mu.data_ptr() == mean.data_ptr()
            actions = st.act(xo, xc, mu, std, values).clone()
            if clip is not None:
                actions = actions.clamp(-clip, clip)
        torch.cuda.synchronize()
        for name in SLOT_NAMES:
            assert bool((getattr(st, name)[1] == SENTINEL).all()), f"{name}: written behind row {N}"
        assert bool((act_out[N:] == SENTINEL).all()) and bool((mean[N:] == SENTINEL).all())
        out = {name: getattr(st, name)[0].clone() for name in SLOT_NAMES}
        out["actions_out"], out["mean"] = actions, mean[:N].clone()
        st.close()
        return out

    a, b = side(True), side(False)
    for name in a:
        assert torch.equal(a[name], b[name]), f"{name} differs (max |d| {float((a[name] - b[name]).abs().max()):.3e})"
        assert not bool((a[name] == SENTINEL).any()), f"{name}: rows left unwritten"
    assert torch.equal(a["observations"], xo) and torch.equal(a["privileged_observations"], xc) and torch.equal(a["mu"], a["mean"])
    if clip is not None:
        assert float(a["actions_out"].abs().max()) <= float(np.float32(clip))  # (the kernel clamps to the fp32 clip)
    actor.close()
    critic.close()
