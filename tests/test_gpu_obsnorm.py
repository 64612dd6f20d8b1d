"""`-m gpu`: the observation-normalisation kernels (include/rl_obsnorm.h, csrc/rl_obsnorm.hip, robot_lab_amd/obsnorm.py) against the rule of
robot_lab_amd.ppo.EmpiricalNormalization as tests/obsnorm_helpers.py restates it in fp64.  Exact tier: no tolerance.  Bounded tier:
max |state - fp64 rule| <= K x the fp32 numpy rule's own distance from the fp64 rule, per state vector; K and where it comes from are in the
helpers, the measured ratios in profiles/obsnorm_accuracy.txt (this file prints the lines)."""
import ctypes as C

import numpy as np
import pytest

import obsnorm_helpers as oh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _norm(dim, max_rows=4096, eps=oh.EPS):
    from robot_lab_amd.obsnorm import ObsNormalizer

    return ObsNormalizer(dim, eps, max_rows=max_rows, device=DEV)


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _state(h):
    mean, var, std, count = h.get_state()
    return dict(mean=mean.cpu().numpy().reshape(-1), var=var.cpu().numpy().reshape(-1), std=std.cpu().numpy().reshape(-1), count=count)


def _set(h, state):
    h.set_state(_dev(state["mean"]), _dev(state["var"]), _dev(state["std"]), state["count"])


def _assert_state_bits(got, want, what):
    assert got["count"] == want["count"], f"{what}: count {got['count']} != {want['count']}"
    for k in oh.VECTORS:
        oh.assert_bits_equal(got[k], np.asarray(want[k]).astype(np.float32), f"{what}, {k}")


@pytest.mark.parametrize("dim", oh.DIMS)
def test_exact_family_equals_the_fp64_rule_bit_for_bit(dim):
    """integer inputs times powers of two, 64 and 256 rows, one and two updates: nothing rounds (asserted by the helper before anything runs),
    so the device state is the fp64 rule's, bit for bit, with an exact count and a variance of exactly 0 in the constant column"""
    h, cases = _norm(dim), 0
    for rows in oh.EXACT_ROWS:
        for updates in (1, 2):
            start, batches, states = oh.exact_batches(rows, dim, updates, seed=rows + dim + updates)
            _set(h, start)
            for u, x in enumerate(batches):
                h.update(_dev(x))
                got = _state(h)
                _assert_state_bits(got, states[u], f"{rows}x{dim}, update {u + 1} of {updates}")
                assert got["var"][0] == 0.0 and got["std"][0] == 0.0 and got["mean"][0] == states[u]["mean"][0]
            cases += 1
    assert cases == 4
    h.close()


@pytest.mark.parametrize("dim", oh.DIMS)
def test_apply_equals_numpys_fp32_bits(dim):
    """y = (x - mean) / (std + eps), three fp32 roundings, on every row count: from a fresh handle, from random states given through the set
    call, after an update (the state the stream finds), in place, and over T N = 24 x 300 rows"""
    import torch

    rng = np.random.default_rng(dim)
    h = _norm(dim)
    for i, rows in enumerate(oh.ROWS + (7200,)):
        x = oh.bounded_batches(rows, dim, 1, seed=rows + dim)[0]
        xd = _dev(x)
        if i % 3 == 1:
            st = dict(mean=rng.uniform(-3, 3, dim).astype(np.float32), var=np.ones(dim, np.float32), std=np.exp(rng.uniform(-9, 2, dim)).astype(np.float32), count=5)
            _set(h, st)
        elif i % 3 == 2 and rows <= 4096:
            h.update(xd)
        st = _state(h)
        want = oh.apply_f32(x, st["mean"], st["std"])
        y = h.apply(xd)
        oh.assert_bits_equal(y.cpu().numpy(), want, f"apply {rows}x{dim}")
        assert torch.equal(xd.cpu(), torch.from_numpy(x))  # the input is not touched
        h.apply(xd, out=xd)
        oh.assert_bits_equal(xd.cpu().numpy(), want, f"apply in place {rows}x{dim}")
    h.close()


@pytest.mark.parametrize("da,db", [(45, 235), (235, 45), (1, 512), (47, 3)])
def test_a_pair_call_equals_two_single_calls(da, db):
    import torch

    for rows in oh.ROWS:
        xa, xb = (_dev(b) for b in (oh.bounded_batches(rows, da, 1, seed=rows)[0], oh.bounded_batches(rows, db, 1, seed=rows + 1)[0]))
        a1, b1, a2, b2 = _norm(da), _norm(db), _norm(da), _norm(db)
        for _ in range(2):
            a1.update(xa)
            b1.update(xb)
            a2.update_pair(xa, b2, xb)
        for one, two in ((a1, a2), (b1, b2)):
            _assert_state_bits(_state(two), _state(one), f"update_pair {rows} rows, {da} / {db}")
        ya, yb = a1.apply(xa), b1.apply(xb)
        pa, pb = a2.apply_pair(xa, b2, xb)
        assert torch.equal(ya.view(torch.int32), pa.view(torch.int32)) and torch.equal(yb.view(torch.int32), pb.view(torch.int32)), (rows, da, db)
        for h in (a1, b1, a2, b2):
            h.close()


def _sequence(h, batches, probe, out):
    for x in batches:
        h.update(x)
    h.apply(probe, out=out)


@pytest.mark.parametrize("dim,rows", [(45, (4096, 257, 65, 1)), (512, (63, 64, 4096))])
def test_same_bits_again_and_from_a_captured_graph(dim, rows):
    """no floating-point atomics and a merge in tile order: a second run of the same sequence gives the same bits, whichever workgroup arrives
    last; nothing is allocated after create and the ticket rearms itself: the sequence replays from a captured graph, twice, with the same bits"""
    import torch

    batches = [_dev(oh.bounded_batches(r, dim, 1, seed=r)[0]) for r in rows]
    probe = batches[0]
    runs = []
    for _ in range(2):
        h, out = _norm(dim), torch.empty_like(probe)
        _sequence(h, batches, probe, out)
        runs.append((_state(h), out.cpu().numpy()))
        h.close()
    _assert_state_bits(runs[1][0], runs[0][0], "second run")
    oh.assert_bits_equal(runs[1][1], runs[0][1], "second run, apply")
    h, out = _norm(dim), torch.empty_like(probe)
    fresh = oh.fresh(dim, np.float32)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _sequence(h, batches, probe, out)
    for replay in range(2):
        _set(h, fresh)
        out.zero_()
        g.replay()
        _assert_state_bits(_state(h), runs[0][0], f"graph replay {replay}")
        oh.assert_bits_equal(out.cpu().numpy(), runs[0][1], f"graph replay {replay}, apply")
    h.close()


def test_zero_rows_change_nothing_and_launch_nothing():
    import torch

    h = _norm(45)
    h.update(_dev(oh.bounded_batches(65, 45, 1, seed=0)[0]))
    before, launches = _state(h), h.lib.rl_obsnorm_launch_count()
    empty = torch.empty(0, 45, device=DEV)
    h.update(empty)
    assert h.apply(empty).shape == (0, 45)
    assert h.lib.rl_obsnorm_launch_count() == launches
    _assert_state_bits(_state(h), before, "n_rows == 0")
    h.close()


def test_bounded_family_stays_within_the_fp32_reference_bound():
    """ROWS x DIMS, one to four consecutive updates of the bounded family (columns with mean 1e3 / std 1e-2, mean 0 / std 1e-4, constant but
    for one row): per state vector and shape E = max |state - fp64 rule| <= K_STATE x E32, E32 the fp32 numpy rule's distance from the same
    fp64 rule, both maxima over the shape's draws and updates (tests/obsnorm_helpers.py says why)."""
    bad, worst = [], 0.0
    for dim in oh.DIMS:
        h = _norm(dim)
        for rows in oh.ROWS:
            e, e32 = dict.fromkeys(oh.VECTORS, 0.0), dict.fromkeys(oh.VECTORS, 0.0)
            for seed in range(oh.BOUND_SEEDS):
                batches, refs, emus = oh.bound_case(rows, dim, 1000 * dim + rows + 7919 * seed)
                _set(h, oh.fresh(dim, np.float32))
                for u, x in enumerate(batches):
                    h.update(_dev(x))
                    got = _state(h)
                    assert got["count"] == rows * (u + 1)
                    for k in oh.VECTORS:
                        e[k], e32[k] = max(e[k], oh.vector_error(got, refs[u], k)), max(e32[k], oh.vector_error(emus[u], refs[u], k))
            for k in oh.VECTORS:
                assert e32[k] > 0.0, f"{rows}x{dim} {k}: the fp32 numpy rule is exact here - no yardstick"
                ratio = e[k] / e32[k]
                print(f"[obsnorm-accuracy] {rows}x{dim} {k} {e[k]:.3e} {e32[k]:.3e} {ratio:.3f}")
                worst = max(worst, ratio)
                if not ratio <= oh.K_STATE:
                    bad.append((rows, dim, k, e[k], e32[k]))
        h.close()
    print(f"[obsnorm-accuracy] largest ratio {worst:.3f}, K_STATE {oh.K_STATE:g}")
    assert not bad, f"state error above {oh.K_STATE:g} x the fp32 numpy rule's: {bad[:8]}"


def test_refusals_name_their_reason_and_launch_nothing():
    import torch

    from robot_lab_amd.obsnorm import ObsNormalizer, RlObsNormError, load_obsnorm_library

    lib = load_obsnorm_library()
    launches = lib.rl_obsnorm_launch_count()
    for dim in (0, 513):
        with pytest.raises(RlObsNormError, match="dim must be 1 .. 512"):
            ObsNormalizer(dim, device=DEV)
    out = C.c_void_p()
    assert lib.rl_obsnorm_create(45, 1e-2, 0, 0, C.byref(out)) == -1 and b"max_rows" in lib.rl_obsnorm_last_error()
    assert lib.rl_obsnorm_create(45, 1e-2, 64, 0, None) == -1 and b"NULL" in lib.rl_obsnorm_last_error()
    h, other = _norm(45, max_rows=64), _norm(7, max_rows=128)
    x = torch.zeros(65, 45, device=DEV)
    before = _state(h)
    with pytest.raises(RlObsNormError, match="max_rows"):
        h.update(x)
    with pytest.raises(RlObsNormError, match="max_rows"):
        other.update_pair(torch.zeros(65, 7, device=DEV), h, x)
    p, null, stream = C.c_void_p(x.data_ptr()), C.c_void_p(), C.c_void_p()
    for rc in (lib.rl_obsnorm_update(h.handle, null, 8, stream), lib.rl_obsnorm_update(null, p, 8, stream), lib.rl_obsnorm_apply(h.handle, p, null, 8, stream),
               lib.rl_obsnorm_apply(h.handle, null, p, 8, stream), lib.rl_obsnorm_update_pair(h.handle, p, null, p, 8, stream),
               lib.rl_obsnorm_update_pair(h.handle, p, other.handle, null, 8, stream), lib.rl_obsnorm_apply_pair(h.handle, p, p, other.handle, p, null, 8, stream),
               lib.rl_obsnorm_state_pointers(null, None, None, None, None), lib.rl_obsnorm_set_state(null, None, None, None, 0, stream)):
        assert rc == -1 and b"NULL" in lib.rl_obsnorm_last_error()
    assert lib.rl_obsnorm_update(h.handle, p, -1, stream) == -1 and b"negative" in lib.rl_obsnorm_last_error()
    with pytest.raises(RlObsNormError, match="contiguous fp32"):
        h.update(torch.zeros(8, 44, device=DEV))
    assert lib.rl_obsnorm_launch_count() == launches
    _assert_state_bits(_state(h), before, "after the refusals")
    h.close()
    other.close()
