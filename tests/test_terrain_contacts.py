"""CPU tier of the off-the-platform parity checks (tests/terrain_helpers.py): the lane program - the CPU lane emulator, the very source
hipcc compiles - against the fp64 oracle, one teacher-forced step from robots PLACED over a hash-coded heightfield, on sinusoidal waves,
mid-slope, across stair risers, tile seams and the grid's edges.  What no reset-and-walk test reaches: the fp64
base / fp32 offset split of the lookups with floorf on negative offsets, the cell and fraction clamps, the (ix, iy) addressing, the x and
y components of the normal, tilted normals in the contact solve.  The GPU tier is tests/test_gpu_terrain_contacts.py."""
import numpy as np
import pytest

import terrain_helpers as th

# (task, RL_EMU_SUB, envs): A1 in the 4-lane and the 16-lane mapping, Go2W (wheels, the merged instance), G1 in the 32-lane mapping, and the task
# whose base_height_l2 has a weight (its 3 x 3 ray caster).  Several lanes per limb run as fibers of one host thread (RL_EMU_FIBERS=1, as
# tests/test_emu_vs_oracle.py runs the trunk + limbs instances): 64 envs x 16 host threads take ten times as long for the same numbers.
CASES = [(th.A1, None, 64), (th.A1, "4", 64), (th.GO2W, "4", 64), (th.G1, "8", 32), (th.TITA, None, 64)]


def _emu(task, sub, monkeypatch):
    if sub is not None:
        monkeypatch.setenv("RL_EMU_SUB", sub)
        monkeypatch.setenv("RL_EMU_FIBERS", "1")
    return f"{task}/emu"


@pytest.mark.parametrize("family", list(th.FAMILIES))
@pytest.mark.parametrize("task,sub,N", CASES)
def test_placed_robots_match_the_oracle(task, sub, N, family, emu_lib, monkeypatch):
    """Checks (a), (b) and (c) of tests/terrain_helpers.py; the switch mask's cap (1 / 8 of the family) is asserted on the oracle alone,
    before anything is compared."""
    key = _emu(task, sub, monkeypatch)
    field, _, mutate, _ = th.FAMILIES[family]
    desc, h, to = th.make_world(task, N, field, mutate)
    drv = th.Driver(desc, h, to, N, 42, emu_lib)
    ora = th.oracle_for(desc, h, to, N, 42)
    if sub == "8":
        assert drv.nat.envs_per_wavefront() == 2
    rep = th.run_case(family, drv, ora, key=key)
    print("\n[terrain-parity]", th.profile_line(task, "emu" + (sub or "1"), rep), rep.get("claims"))
    drv.close()


# defect of the lookup -> (family, check) that catches it.  (a): teacher_forced_check + contact forces; (b): the lookup alone.
TEETH = dict(swap_index=("interior", "b"), cell_plus_one=("lattice", "b"), clamp_nx_1=("edges", "b"), fraction_unclamped=("edges", "b"),
             swap_normal=("waves", "a"), dzdy_sign=("slopes", "a"))


@pytest.mark.parametrize("defect", list(TEETH))
def test_the_checks_have_teeth(defect):
    """No kernel involved: the oracle with a DEFECTIVE copy of TerrainSampler (th.DefectiveSampler) in the tested side's place, the sound one on
    the other.  x and y swapped in the index -> `interior` fails check (b); the cell off by one -> `lattice`, (b); the cell clamped to nx - 1
    (reads past the last row / column) and the fraction not clamped outside the grid -> `edges`, (b); x and y swapped in the normal ->
    `waves`, (a); dz/dy with the wrong sign -> `slopes`, (a).  A defect no family catches would mean a family is missing."""
    family, check = TEETH[defect]
    N = 64
    field, _, mutate, _ = th.FAMILIES[family]
    desc, h, to = th.make_world(th.A1, N, field, mutate)
    ora = th.oracle_for(desc, h, to, N, 42)
    bad = th.OracleDriver(th.oracle_for(desc, h, to, N, 42, th.DefectiveSampler(desc.terrain, h, defect)))
    with pytest.raises(AssertionError, match=rf"check \({check}\) {family}"):
        th.run_case(family, bad, ora, checks=(check,), key=f"{th.A1}/teeth")


def test_the_sound_sampler_passes_the_same_checks():
    """... and the same stand-in with the SOUND sampler passes both checks: what fails above is the defect, not the stand-in."""
    N = 64
    for family in ("edges", "waves"):
        field, _, mutate, _ = th.FAMILIES[family]
        desc, h, to = th.make_world(th.A1, N, field, mutate)
        rep = th.run_case(family, th.OracleDriver(th.oracle_for(desc, h, to, N, 42)), th.oracle_for(desc, h, to, N, 42), key=f"{th.A1}/teeth")
        assert rep["b"]["ratio"] < 1.0, rep["b"]  # (fp32 state exchange, fp64 arithmetic: far inside one unit)


def test_the_fields_are_what_they_claim():
    """`coded`: bounded, no two neighbouring nodes alike, different along x and along y, non-zero on the border strip and in the last row and
    column; `waves`: slopes of a few tenths, the x and y gradients different in size and sign over most of the field."""
    nx, ny = 2401, 4001
    c = th.coded_field(nx, ny).astype(np.float64)
    mesa = th.is_mesa(*np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"))
    assert np.abs(c[~mesa]).max() <= th.CODED_AMP and c.max() <= th.MESA_HEIGHT + th.CODED_AMP
    assert (np.abs(np.diff(c, axis=0)) > 1e-4).mean() > 0.99 and (np.abs(np.diff(c, axis=1)) > 1e-4).mean() > 0.99
    assert np.abs(c[:2000, :2000] - c[:2000, :2000].T).mean() > 0.01  # ix for iy shows
    assert np.abs(c[:-1].reshape(-1)[: nx * 100] - c.T.reshape(-1)[: nx * 100]).mean() > 0.01  # ... and so does the row stride nx for ny
    for strip in (c[:400], c[-400:], c[:, :400], c[:, -400:], c[-1:], c[:, -1:]):
        assert np.abs(strip).mean() > 0.01
    w = th.waves_field(nx, ny).astype(np.float64)
    gx, gy = np.diff(w, axis=0)[:, :-1] / 0.05, np.diff(w, axis=1)[:-1] / 0.05
    assert 0.5 < np.hypot(gx, gy).max() < 1.0 and np.median(np.hypot(gx, gy)) > 0.2
    assert (np.abs(np.abs(gx) - np.abs(gy)) > 0.05).mean() > 0.7 and 0.3 < (np.sign(gx) != np.sign(gy)).mean() < 0.7
    for strip in (w[:400], w[-400:], w[:, :400], w[:, -400:]):
        assert np.abs(strip).mean() > 0.05


def test_fp64_lane_program_on_the_placements():
    """The lane program retyped to double (tests/emu/make_f64.py, as tests/test_fp64_lane_program.py) on the same placements: every family,
    A1 in the 4-lane mapping, state and observations to 1e-9 relative, contact forces to 1e-6 N (measured: <= 7e-11, 3e-10 N).  In double
    nothing hides inside an envelope or a margin - the lookups' algorithm IS the oracle's rule, and what the fp32 checks above leave is
    round-off."""
    import json
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "emu"))
    import make_f64

    lib = make_f64.build()
    out = subprocess.run([sys.executable, os.path.join(here, "fp64_terrain_families.py"), th.A1, "64", lib], env=dict(os.environ, RL_ABI_REAL="f64"),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rep = json.loads([l for l in out.stdout.splitlines() if l.startswith("FP64_TERRAIN ")][-1][len("FP64_TERRAIN "):])
    assert set(rep) == set(th.FAMILIES)
    for family, r in rep.items():
        assert all(r[f] <= 1e-9 for f in ("root_state", "joint_pos", "joint_vel", "obs_policy", "obs_critic")) and r["contact_force_abs"] <= 1e-6, (family, r)
        assert r["masked"] <= 8 and (r["contact_force_max"] > 20.0) == (family in ("slopes", "stairs", "seams", "waves")), (family, r)
