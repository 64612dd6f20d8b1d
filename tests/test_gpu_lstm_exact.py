"""The LSTM cell kernel (robot_lab_amd/csrc/rl_lstm.hip, include/rl_lstm.h) on the MI355X: exact families with no tolerance (integer
pre-activations at every tile edge, saturated gates, resets over NaN), the fp32-referenced bound of a 24-step unroll, and the launch
equivalences (pair = two singles, NULL outputs, device push = create, aliasing refused).  Helpers and case tables:
tests/recurrent_helpers.py; their CPU side: tests/test_recurrent.py."""
import numpy as np
import pytest

import recurrent_helpers as rh
from policy_helpers import assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = rh.DEV


def _dev(a, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


def _cell(params):
    from robot_lab_amd.lstm import LstmCell

    return LstmCell(*params, device=DEV)


def _step(cell, x, h, c, reset=None, saved=True, gates=True):
    """one launch; dict of numpy outputs (None where the output was not asked for)"""
    import torch

    n, H = x.shape[0], cell.hidden
    new = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out = dict(h=new(n, H), c=new(n, H), h_saved=new(n, H) if saved else None, c_saved=new(n, H) if saved else None, z=new(n, 4 * H) if gates else None)
    cell.step(_dev(x), _dev(h), _dev(c), out["h"], out["c"], reset=None if reset is None else _dev(reset, np.uint8), h_saved=out["h_saved"],
              c_saved=out["c_saved"], gates_out=out["z"])
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("N,D,H", rh.INTEGER_CASES)
def test_integer_pre_activations_are_exact(N, D, H):
    """integer weights, inputs and states: `gates_out` equals the int64 z; every row, k and unit tile edge of the kernel is in the case table"""
    x, h, c, params, z = rh.integer_case(N, D, H, seed=N + D + H)
    cell = _cell(params)
    got = _step(cell, x, h, c)
    assert got["z"].shape == (N, 4 * H)
    assert np.array_equal(got["z"].astype(np.int64), z), f"{int((got['z'].astype(np.int64) != z).sum())} of {z.size} pre-activations differ"
    assert_bits_equal(got["h_saved"], h, "h_saved without a reset")
    assert_bits_equal(got["c_saved"], c, "c_saved without a reset")
    assert np.isfinite(got["h"]).all() and np.isfinite(got["c"]).all()
    cell.close()


@pytest.mark.parametrize("N,D,H", [(37, 45, 256), (33, 7, 20), (16, 235, 129)])
def test_saturated_gates_are_exact(N, D, H):
    x, h, c, params = rh.saturated_case(N, D, H, seed=5)
    reset = (np.arange(N) % 3 == 0)
    h_in, c_in = h.copy(), c.copy()
    h_in[reset], c_in[reset] = np.nan, np.nan  # a reset row's old state does not travel, NaN included
    cells = {k: _cell(p) for k, p in params.items()}
    hold = _step(cells["hold"], x, h_in, c_in, reset=reset)
    assert np.abs(hold["z"]).min() >= 128.0 and np.isfinite(hold["z"]).all()
    keep = ~reset
    assert_bits_equal(hold["c"][keep], c[keep], "hold rows: c' is c")
    assert np.all(hold["h"][keep] == 0.0), "hold rows: h' is +-0"
    assert np.all(hold["c"][reset] == 0.0) and np.all(hold["h"][reset] == 0.0), "reset rows under hold gates: c' = 0"
    assert np.all(hold["h_saved"][reset].view(np.uint32) == 0) and np.all(hold["c_saved"][reset].view(np.uint32) == 0), "the saved slot of a reset row is zero"
    assert_bits_equal(hold["h_saved"][keep], h[keep], "non-reset rows: the saved h is the input's bits")
    assert_bits_equal(hold["c_saved"][keep], c[keep], "non-reset rows: the saved c is the input's bits")
    for name, sign in (("write+", 1.0), ("write-", -1.0)):
        got = _step(cells[name], x, h_in, c_in, reset=reset)
        assert np.all(got["c"] == np.float32(sign)), f"{name}: c' = {sign:+.0f} exactly"
        assert_bits_equal(got["h"], np.full_like(c, got["h"][0, 0]), f"{name}: h' = 1 * tanh(+-1), one number for every entry")
        assert abs(float(got["h"][0, 0]) - sign * np.tanh(1.0)) < 1e-6
    for cl in cells.values():
        cl.close()


@pytest.mark.parametrize("D,H", rh.BOUND_CASES)
def test_unroll_within_the_fp32_bound(D, H):
    """24 steps, N = 256, resets on about a tenth of the (row, step) pairs: every saved state, the final state and the last step's gates_out
    within M_BOUND x the fp32 numpy emulation's own distance from the fp64 recursion (tests/recurrent_helpers.py bound_check).
    Measured multiples: profiles/lstm_accuracy.txt."""
    import torch

    params, xs, resets = rh.bound_case(D, H)
    N, T = rh.BOUND_ROWS, rh.BOUND_STEPS
    z0 = np.zeros((N, H))
    r64 = rh.unroll(rh.cell64, xs, resets, params, z0, z0)
    r32 = rh.unroll(rh.cell32, xs, resets, params, z0.astype(np.float32), z0.astype(np.float32))
    cell = _cell(params)
    zt = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    hb, cb = [zt(N, H), zt(N, H)], [zt(N, H), zt(N, H)]
    hs, cs, gates = zt(T, N, H), zt(T, N, H), zt(N, 4 * H)
    xd, rd = _dev(xs), _dev(resets, np.uint8)
    for t in range(T):
        k = t & 1
        cell.step(xd[t], hb[k], cb[k], hb[1 - k], cb[1 - k], reset=rd[t], h_saved=hs[t], c_saved=cs[t], gates_out=gates if t == T - 1 else None)
    torch.cuda.synchronize()
    got = dict(h_saved=hs, c_saved=cs, h=hb[T & 1], c=cb[T & 1], z=gates)
    bad = []
    for k in ("h_saved", "c_saved", "h", "c", "z"):
        ok, line = rh.bound_check(f"D={D} H={H} {k}", got[k].cpu().numpy(), r64[k], r32[k])
        if not ok:
            bad.append(line)
    on = resets[1:].astype(bool)
    assert np.all(hs.cpu().numpy()[1:][on] == 0.0) and np.all(cs.cpu().numpy()[1:][on] == 0.0)
    assert not bad, "\n".join([rh.BOUND_HEADER] + bad)
    cell.close()


def _pair_case():
    pa, pc = rh.lstm_default_init(45, 256, 1), rh.lstm_default_init(235, 64, 2)
    rng = np.random.default_rng(3)
    N = 77
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return pa, pc, N, (f(N, 45), f(N, 256), f(N, 256)), (f(N, 235), f(N, 64), f(N, 64)), rng.random(N) < 0.3


def test_pair_launch_equals_two_single_launches():
    import torch

    pa, pc, N, (xa, ha, ca), (xc, hc, cc), reset = _pair_case()
    a, c = _cell(pa), _cell(pc)
    one_a, one_c = _step(a, xa, ha, ca, reset=reset), _step(c, xc, hc, cc, reset=reset)
    new = lambda H, k=1: torch.full((N, k * H), float("nan"), device=DEV)  # noqa: E731
    oa = dict(h=new(256), c=new(256), h_saved=new(256), c_saved=new(256), z=new(256, 4))
    oc = dict(h=new(64), c=new(64), h_saved=new(64), c_saved=new(64), z=new(64, 4))
    a.step_pair(_dev(xa), _dev(ha), _dev(ca), oa["h"], oa["c"], c, _dev(xc), _dev(hc), _dev(cc), oc["h"], oc["c"], reset=_dev(reset, np.uint8),
                h_saved=oa["h_saved"], c_saved=oa["c_saved"], gates_out=oa["z"], other_h_saved=oc["h_saved"], other_c_saved=oc["c_saved"], other_gates_out=oc["z"])
    torch.cuda.synchronize()
    for name, one, two in (("actor", one_a, oa), ("critic", one_c, oc)):
        for k in one:
            assert_bits_equal(two[k].cpu().numpy(), one[k], f"pair launch, {name} cell, {k}")
    a.close(); c.close()


def test_null_outputs_leave_the_others_bit_identical():
    pa, _, N, (xa, ha, ca), _, reset = _pair_case()
    a = _cell(pa)
    full = _step(a, xa, ha, ca, reset=reset)
    for saved, gates in ((False, True), (True, False), (False, False)):
        part = _step(a, xa, ha, ca, reset=reset, saved=saved, gates=gates)
        for k, v in part.items():
            if v is not None:
                assert_bits_equal(v, full[k], f"saved={saved} gates={gates}: {k}")
    none = _step(a, xa, ha, ca, reset=None, saved=True, gates=False)  # a NULL reset vector resets no row
    zero = _step(a, xa, ha, ca, reset=np.zeros(N, dtype=bool), saved=True, gates=False)
    for k in ("h", "c", "h_saved", "c_saved"):
        assert_bits_equal(none[k], zero[k], f"NULL reset: {k}")
    a.close()


def test_device_push_equals_create():
    import torch

    pa, _, N, (xa, ha, ca), _, reset = _pair_case()
    other = rh.lstm_default_init(45, 256, 9)
    fresh, pushed = _cell(pa), _cell(other)
    before = _step(pushed, xa, ha, ca, reset=reset)
    tensors = [_dev(p) for p in pa]
    pushed.set_weights_device(*tensors)
    torch.cuda.synchronize()
    want, got = _step(fresh, xa, ha, ca, reset=reset), _step(pushed, xa, ha, ca, reset=reset)
    assert not np.array_equal(before["z"], want["z"])
    for k in want:
        assert_bits_equal(got[k], want[k], f"set_weights_device against create: {k}")
    rnn = torch.nn.LSTM(45, 256, 1).to(DEV)
    pushed.load_module(rnn)
    from robot_lab_amd.lstm import LstmCell

    mod = LstmCell.from_module(rnn, device=DEV)
    a, b = _step(pushed, xa, ha, ca), _step(mod, xa, ha, ca)
    for k in a:
        assert_bits_equal(a[k], b[k], f"load_module against from_module: {k}")
    with torch.no_grad():  # nn.LSTM's own layout and gate order: the module itself, on the CPU
        _, (hn, cn) = rnn.cpu()(torch.from_numpy(xa).unsqueeze(0), (torch.from_numpy(ha).unsqueeze(0), torch.from_numpy(ca).unsqueeze(0)))
    # |z| ~ 1 from 301 products: an fp32 sum in another order differs by a few 1e-7; c' = f c + i g carries it times |c| <= 5
    np.testing.assert_allclose(a["h"], hn[0].numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(a["c"], cn[0].numpy(), rtol=0, atol=1e-5)
    for cl in (fresh, pushed, mod):
        cl.close()


def test_aliased_outputs_are_refused():
    import ctypes as C

    import torch

    pa, _, N, (xa, ha, ca), _, _ = _pair_case()
    a = _cell(pa)
    x, h, c = _dev(xa), _dev(ha), _dev(ca)
    o1, o2 = torch.empty_like(h), torch.empty_like(c)
    for kw in (dict(h_out=h, c_out=o2), dict(h_out=o1, c_out=c), dict(h_out=c, c_out=o2), dict(h_out=o1, c_out=o2, h_saved=h), dict(h_out=o1, c_out=o2, c_saved=c)):
        with pytest.raises(ValueError, match="aliases"):
            a.step(x, h, c, kw.pop("h_out"), kw.pop("c_out"), **kw)
    # ... and by the library itself, for a caller that does not come through the binding
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = a.lib.rl_lstm_step(a.handle, p(x), None, p(h), p(c), None, None, p(h), p(o2), None, N, None)
    assert rc != 0 and "aliases" in a.lib.rl_lstm_last_error().decode()
    a.close()
