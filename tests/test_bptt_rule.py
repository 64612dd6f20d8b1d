"""CPU: the backward formulas of include/rl_bptt.h, restated in numpy by hand (tests/bptt_helpers.py `np_block`: no autograd), against torch autograd
through `RecurrentPPO.block_loss` - the teeth of the recurrent learner's GPU parity test (tests/test_gpu_bptt.py), which uses the same bound on the
same shapes and batches.

  - in fp64 the restatement agrees with autograd to 1e-10 relative, per parameter tensor, on every shape and block;
  - in fp32 it passes the project's bound e <= 8 d (d: the fp32 torch rule's own distance from the fp64 torch rule);
  - each of seven wrong rules misses that bound on every block of "ragged" and "4H-crosses-128" that it touches (`-s` prints the tables).
    Recorded: the six gradient defects miss it by 1.5e4 x .. 6.2e5 x (worst tensor of a block, as a multiple of 8 d); the gradient norm that
    leaves db_hh out by 48 x .. 117 x."""
import numpy as np
import pytest

from bptt_helpers import DEFECTS, SHAPES, case, named, np_block, reference_block, within_bound

BLOCKS = [(name, b) for name, s in SHAPES.items() for b in range(s["mb"])]


def _np(name, block, dtype, defect=None):
    pol, f = case(name)
    s = SHAPES[name]
    n = s["N"] // s["mb"]
    return np_block(named(pol), f, block * n, n, dtype=dtype, defect=defect)


@pytest.mark.parametrize("name,block", BLOCKS, ids=[f"{n}-block{b}" for n, b in BLOCKS])
def test_restatement_is_autograd_in_fp64(name, block):
    ref = reference_block(name, block)["f64"]
    mean, value, g = _np(name, block, np.float64)
    assert set(g) == set(ref[2])
    for got, want, what in ((mean, ref[0], "mean"), (value, ref[1], "value")):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), what
    for k, want in ref[2].items():
        scale = np.abs(want).max()
        assert scale > 0, k
        assert np.abs(np.asarray(g[k]).reshape(np.shape(want)) - want).max() <= 1e-10 * scale, (k, np.abs(g[k] - want).max() / scale)


@pytest.mark.parametrize("name,block", BLOCKS, ids=[f"{n}-block{b}" for n, b in BLOCKS])
def test_restatement_in_fp32_passes_the_bound(name, block):
    ref = reference_block(name, block)
    mean, value, g = _np(name, block, np.float32)
    print()
    bad = within_bound(f"{name} block {block}: numpy fp32", dict(g, mean=mean, value=value), dict(ref["f64"][2], mean=ref["f64"][0], value=ref["f64"][1]),
                       dict(ref["f32"][2], mean=ref["f32"][0], value=ref["f32"][1]))
    assert not bad, bad


def _touched(name, block, defect):
    """does the defect change anything on this block at all (a block without a done that matters cannot show a masking defect)"""
    a, b = _np(name, block, np.float64)[2], _np(name, block, np.float64, defect)[2]
    return any(not np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_defect_misses_the_bound(defect):
    """on every block of "ragged" and "4H-crosses-128" that the defect touches - and it touches at least one block of each - some tensor leaves
    the bound, in fp32 arithmetic as the device's"""
    print()
    for name in ("ragged", "4H-crosses-128"):
        hit = 0
        for block in range(SHAPES[name]["mb"]):
            if not _touched(name, block, defect):
                continue
            hit += 1
            ref = reference_block(name, block)
            _, _, g = _np(name, block, np.float32, defect)
            bad = within_bound(f"{name} block {block}: {defect}", g, ref["f64"][2], ref["f32"][2])
            assert bad, f"{defect} stays inside the bound on {name} block {block}: the GPU test could not see it"
            print(f"    -> worst miss: {max(e / (8 * d) if d else np.inf for _, _, e, d in bad):.3g} x the bound ({len(bad)} tensors)")
        assert hit, f"{defect} touches no block of {name}: the done pattern does not exercise it"
