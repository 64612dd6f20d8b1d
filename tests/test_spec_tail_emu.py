"""The scan geometry of a Spec (robot_lab_amd/csrc/env_terms.h spec_scan_slot_xy, env_spec.h SCAN_NX / SCAN_NY / SCAN_RES / SCAN_OFFSET), CPU tier.

A Spec of a quadruped instance with several sub-lanes per limb takes the height scanner's grid from its constants and turns a lane's slot
into a grid point with integer compares; the interpreter reads the grid from the table image and turns the ray index into (ix, iy) with a
float multiply and an int / float round trip.  Two checks, both on a second build of the lane emulator (~2 minutes of g++, once per session):
  * the ray map: for every built-in Spec and a few synthetic grids (rows shorter than an env's lanes, a single column, a grid that fills the
    trip exactly), every lane index and every load of a trip gives the (ix, iy) of the float form, rays behind the grid's last included;
  * one program against the other: the emulator as it ships and built with -DRL_SPEC_SCAN_TABLES (every Spec reads the grid from the
    table image - the stage as it was) give the same words, step by step from a shared state, for each of the eight built-in Specs.
The Spec's program and the INTERPRETER's are not bit-equal on the emulator, before this stage or after it: a Spec composes axis-aligned
joint rotations in their sparse form (tests/test_specs.py holds the two against each other within round-off), so what is held bit for bit
here is the stage with its constants against the stage without them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import STATE_BUFFERS, emu_load_state, emu_read_state, host_view
from robot_lab_amd.capi import NativeEnv
from robot_lab_amd.scene import build_world, load_bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = {  # id -> task (tools/gen_specs.py SPECS)
    1: "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0",
    2: "RobotLab-Isaac-Velocity-Rough-Unitree-Go2-v0",
    3: "RobotLab-Isaac-Velocity-Rough-Unitree-Go2W-v0",
    4: "RobotLab-Isaac-Velocity-Rough-Unitree-G1-v0",
    5: "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0",
    6: "RobotLab-Isaac-Velocity-Flat-Unitree-Go2-v0",
    7: "RobotLab-Isaac-Velocity-Flat-Unitree-Go2W-v0",
    8: "RobotLab-Isaac-Velocity-Flat-Unitree-G1-v0",
}
SYNTHETIC = {101: (5, 7), 102: (33, 3), 103: (16, 12), 104: (1, 9), 105: (17, 11)}  # id -> (nx, ny) of the wrapper's grids
OUTPUTS = ("OBS_POLICY", "OBS_CRITIC", "REWARD", "REWARD_TERMS", "TERMINATED", "TIME_OUT")
TRIP = 12  # loads of a lane per trip (env_terms.h SCAN_RB with up to 16 lanes per env)

WRAPPER = """// the lane emulator with every Spec reading the scanner's grid from the table image (-DRL_SPEC_SCAN_TABLES) + the slot -> grid point map
#include "%s"
namespace {
template <int NX, int NY>
struct Grid {
  static constexpr int SCAN_NX = NX, SCAN_NY = NY;
};
template <class SP, int LPE>
void fill(int* out) {
  rl::static_for<0, %d>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    for (int li = 0; li < LPE; ++li) rl::spec_scan_slot_xy<SP, LPE, I>(li, out[(I * LPE + li) * 2], out[(I * LPE + li) * 2 + 1]);
  });
}
template <class SP>
int fill_lpe(int lpe, int* out, int* grid) {
  grid[0] = SP::SCAN_NX; grid[1] = SP::SCAN_NY;
  if (lpe == 8) fill<SP, 8>(out);
  else if (lpe == 16) fill<SP, 16>(out);
  else if (lpe == 32) fill<SP, 32>(out);
  else return -1;
  return 0;
}
}  // namespace
extern "C" int rl_test_scan_map(int id, int lpe, int* out, int* grid) {
#define RL_TEST_X(NAME, ID) if (id == ID) return fill_lpe<rl::NAME>(lpe, out, grid);
  RL_SPEC_LIST(RL_TEST_X)
#undef RL_TEST_X
  if (id == 101) return fill_lpe<Grid<5, 7>>(lpe, out, grid);
  if (id == 102) return fill_lpe<Grid<33, 3>>(lpe, out, grid);
  if (id == 103) return fill_lpe<Grid<16, 12>>(lpe, out, grid);
  if (id == 104) return fill_lpe<Grid<1, 9>>(lpe, out, grid);
  if (id == 105) return fill_lpe<Grid<17, 11>>(lpe, out, grid);
  return -1;
}
"""


@pytest.fixture(scope="session")
def tables_lib(tmp_path_factory, emu_lib):
    d = tmp_path_factory.mktemp("emu_scan_tables")
    src, out = d / "emu_scan_tables.cpp", str(d / "librl_env_emu_scan_tables.so")
    src.write_text(WRAPPER % (os.path.join(ROOT, "tests", "emu", "rl_env_emu.cpp"), TRIP))
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-DRL_SPEC_SCAN_TABLES", "-o", out, str(src)], check=True)
    return out


def float_form(slots, nx, ny):
    """(ix, iy) of the slots' rays as the interpreter computes them (env_terms.h scan_fetch_trip), in fp32"""
    r = np.minimum(slots, nx * ny - 1).astype(np.int32)
    inv = np.float32(1.0) / np.float32(nx)
    iy = ((r.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
    return r - iy * nx, iy


@pytest.mark.parametrize("gid", sorted(SPECS) + sorted(SYNTHETIC))
def test_ray_map_equals_the_float_form(gid, tables_lib):
    hook = ctypes.CDLL(tables_lib)
    hook.rl_test_scan_map.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    for lpe in (8, 16, 32):
        out = np.full((TRIP, lpe, 2), -1, dtype=np.int32)
        grid = np.zeros(2, dtype=np.int32)
        assert hook.rl_test_scan_map(gid, lpe, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), grid.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
        nx, ny = int(grid[0]), int(grid[1])
        if gid in SYNTHETIC:
            assert (nx, ny) == SYNTHETIC[gid]
        slots = np.arange(lpe)[None, :] + lpe * np.arange(TRIP)[:, None]  # slot of lane li in its i-th load
        ix, iy = float_form(slots, nx, ny)
        assert np.array_equal(out[..., 0], ix) and np.array_equal(out[..., 1], iy), (gid, lpe, nx, ny)
        live = slots < nx * ny  # every ray of the grid that a trip of this width reaches stands in the slot of its index
        assert np.array_equal((out[..., 1] * nx + out[..., 0])[live], slots[live])


@pytest.mark.parametrize("sid,sub", [(1, 4), (1, 2), (2, 4), (3, 4), (3, 2), (4, 8), (5, 4), (6, 4), (7, 4), (8, 8)])
def test_spec_constants_program_equals_table_image_program_word_for_word(sid, sub, emu_lib, tables_lib, monkeypatch):
    monkeypatch.setenv("RL_EMU_FIBERS", "1")  # deterministic: the trunk + limbs instance adds into shared words (thread order otherwise)
    monkeypatch.setenv("RL_EMU_SUB", str(sub))
    monkeypatch.setenv("RL_ENV_SPEC", "1")
    task, N, steps = SPECS[sid], 5, 3
    desc, extra = load_bundle(task)
    h, to, eo = build_world(desc, extra, N, 0)
    a = NativeEnv(desc, h, to, eo, N, 5, 0, emu_lib)
    b = NativeEnv(desc, h, to, eo, N, 5, 0, tables_lib)
    assert a.spec_id() == sid and b.spec_id() == sid
    a.reset(); b.reset()
    rng = np.random.default_rng(0)
    for s in range(steps):
        act = (rng.random((N, a.num_actions), dtype=np.float32) * 2 - 1).astype(np.float32)
        emu_load_state(b, emu_read_state(a))
        a.step(act.ctypes.data); b.step(act.ctypes.data)
        for name in OUTPUTS:
            assert host_view(a, name).tobytes() == host_view(b, name).tobytes(), (task, sub, s, name)
        sa, sb = emu_read_state(a), emu_read_state(b)
        for k in STATE_BUFFERS:
            assert sa[k.lower()].tobytes() == sb[k.lower()].tobytes(), (task, sub, s, k)
    if sid <= 4:  # the Rough tasks carry the scan in the critic row: it is not a row of constants
        scan = host_view(a, "OBS_CRITIC")[:, -187:]
        assert np.unique(scan).size > 20


def test_a_grid_the_spec_does_not_know_keeps_the_interpreter(emu_lib, monkeypatch):
    """spec_matches: a descriptor whose scanner grid or offset differs from the Spec's constants runs the interpreter."""
    monkeypatch.setenv("RL_ENV_SPEC", "1")
    task = SPECS[1]

    def make(mutate):
        desc, extra = load_bundle(task)
        if mutate is not None:
            mutate(desc)
        h, to, eo = build_world(desc, extra, 4, 0)
        return NativeEnv(desc, h, to, eo, 4, 1, 0, emu_lib)

    def finer(desc):
        desc.task.scan_res = 0.05

    def lower(desc):
        desc.task.scan_offset = 0.4

    assert make(None).spec_id() == 1
    assert make(finer).spec_id() == 0
    assert make(lower).spec_id() == 0
