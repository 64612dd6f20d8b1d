"""The sphere-slot census of a Spec (robot_lab_amd/csrc/env_spec.h SLOT_VALID / spec_slot_any), CPU tier.

A Spec's step program drops, at compile time, every collision-sphere slot that no link group of its task fills.  That is only right
when the constant it was generated with IS the `slot_valid` word of the host tables, and it may not change a single bit of a result: an
empty slot evaluates to phi = -1, no contact, no force.  Two checks:
  * for every bundled task, the SLOT_VALID in the task's Spec source (and, for the eight built-in Specs, in csrc/spec/env_specs_gen.h)
    equals the slot_valid word `compile_tables` computes from the task's descriptor; a descriptor with one more sphere no longer
    matches its Spec;
  * the lane emulator built as it ships (census on) and built with -DRL_SLOT_VALID_ALL (every Spec walks every slot, as the
    interpreter does) give the same words - outputs and state - step by step from a shared state, with feet on the ground.
Both need a second emulator build (~2 minutes of g++, once per session): the wrapper below includes tests/emu/rl_env_emu.cpp and adds
a hook that returns the host tables' word."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import STATE_BUFFERS, emu_load_state, emu_read_state, host_view
from robot_lab_amd.capi import NativeEnv
from robot_lab_amd.desc import EnvDesc
from robot_lab_amd.scene import build_world, load_bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "robot_lab_amd", "data")
TASKS = sorted(f[:-5] for f in os.listdir(DATA) if f.startswith("RobotLab-Isaac-") and f.endswith(".json"))
SPECS = {  # id -> (struct, task): tools/gen_specs.py SPECS
    1: ("Spec_A1_Rough", "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0"),
    2: ("Spec_Go2_Rough", "RobotLab-Isaac-Velocity-Rough-Unitree-Go2-v0"),
    3: ("Spec_Go2W_Rough", "RobotLab-Isaac-Velocity-Rough-Unitree-Go2W-v0"),
    4: ("Spec_G1_Rough", "RobotLab-Isaac-Velocity-Rough-Unitree-G1-v0"),
    5: ("Spec_A1_Flat", "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"),
    6: ("Spec_Go2_Flat", "RobotLab-Isaac-Velocity-Flat-Unitree-Go2-v0"),
    7: ("Spec_Go2W_Flat", "RobotLab-Isaac-Velocity-Flat-Unitree-Go2W-v0"),
    8: ("Spec_G1_Flat", "RobotLab-Isaac-Velocity-Flat-Unitree-G1-v0"),
}
OUTPUTS = ("OBS_POLICY", "OBS_CRITIC", "REWARD", "REWARD_TERMS", "TERMINATED", "TIME_OUT")

WRAPPER = """// the lane emulator with every Spec walking every sphere slot (-DRL_SLOT_VALID_ALL) + the host tables' slot_valid word of a descriptor
#include "%s"
extern "C" long long rl_test_slot_valid(const rl_env_desc* d) {
  rl::Tables* T = new rl::Tables();
  std::vector<int> bl, bs, ll, lp;
  const long long w = rl::compile_tables(*d, *T, bl, bs, ll, lp) ? -1 : (long long)T->slot_valid;
  delete T;
  return w;
}
"""


@pytest.fixture(scope="session")
def allslots_lib(tmp_path_factory, emu_lib):
    d = tmp_path_factory.mktemp("emu_allslots")
    src, out = d / "emu_allslots.cpp", str(d / "librl_env_emu_allslots.so")
    src.write_text(WRAPPER % os.path.join(ROOT, "tests", "emu", "rl_env_emu.cpp"))
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-DRL_SLOT_VALID_ALL", "-o", out, str(src)], check=True)
    return out


def _desc(task, mutate=None):
    desc, extra = load_bundle(task)
    if mutate is not None:
        mutate(desc)
    build_world(desc, extra, 16, 0)
    return desc


def _source(lib, desc, task):
    buf = ctypes.create_string_buffer(1 << 17)
    n = lib.rl_env_spec_source(ctypes.byref(desc), b"Spec_T", task.encode(), 1000, buf, len(buf))
    return buf.value.decode() if n > 0 else None


def _slot_valid_of(src):
    m = re.findall(r"static constexpr uint32_t SLOT_VALID = 0x([0-9a-f]+)u;", src)
    assert len(m) == 1, m
    return int(m[0], 16)


def test_spec_constant_is_the_host_tables_word(emu_lib, allslots_lib):
    lib, hook = ctypes.CDLL(emu_lib), ctypes.CDLL(allslots_lib)
    lib.rl_env_spec_source.argtypes = [ctypes.POINTER(EnvDesc), ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    hook.rl_test_slot_valid.argtypes = [ctypes.POINTER(EnvDesc)]
    hook.rl_test_slot_valid.restype = ctypes.c_longlong
    assert len(TASKS) >= 40
    words, compared = {}, 0
    for task in TASKS:
        desc = _desc(task)
        words[task] = hook.rl_test_slot_valid(ctypes.byref(desc))
        assert words[task] > 0, task  # (compiled, and some sphere exists)
        src = _source(lib, desc, task)
        if src is None:  # a task the specialised evaluation cannot express has no Spec and no census to get wrong
            continue
        assert _slot_valid_of(src) == words[task], (task, hex(_slot_valid_of(src)), hex(words[task]))
        compared += 1
    assert compared >= 40, compared
    gen = open(os.path.join(ROOT, "robot_lab_amd", "csrc", "spec", "env_specs_gen.h")).read()
    for sid, (name, task) in SPECS.items():
        body = gen[gen.index(f"struct {name} {{"):]
        body = body[: body.index("\n};\n")]
        assert _slot_valid_of(body) == words[task], (name, hex(words[task]))
    # what the issue of this census rests on: A1 fills two of the three slots of every link group, in every limb
    assert words[SPECS[1][1]] == 0b011_011_011_011


def test_a_sphere_the_spec_does_not_know_keeps_the_interpreter(emu_lib, monkeypatch):
    """One more collision sphere on an A1 calf fills the slot the Spec's kernel does not walk: the tables no longer match the Spec."""
    monkeypatch.setenv("RL_ENV_SPEC", "1")
    task = SPECS[1][1]

    def make(mutate):
        desc, extra = load_bundle(task)
        if mutate is not None:
            mutate(desc)
        h, to, eo = build_world(desc, extra, 4, 0)
        return NativeEnv(desc, h, to, eo, 4, 1, 0, emu_lib)

    def third_sphere(desc):
        m = desc.model
        g, last = m.num_spheres, m.num_spheres - 1  # a copy of the last sphere (a foot), a little smaller, on the same body
        m.sphere_body[g] = m.sphere_body[last]
        for c in range(3):
            m.sphere_center[g][c] = m.sphere_center[last][c]
        m.sphere_radius[g] = 0.5 * m.sphere_radius[last]
        m.num_spheres = g + 1

    assert make(None).spec_id() == 1
    assert make(third_sphere).spec_id() == 0


@pytest.mark.parametrize("sid,sub", [(1, 4), (1, 2), (1, 1), (2, 4), (2, 1), (3, 4), (4, 8), (5, 4), (6, 4), (7, 4), (8, 8)])
def test_census_program_equals_all_slots_program_word_for_word(sid, sub, emu_lib, allslots_lib, monkeypatch):
    monkeypatch.setenv("RL_EMU_FIBERS", "1")  # deterministic: the trunk + limbs instance adds into shared words (thread order otherwise)
    monkeypatch.setenv("RL_EMU_SUB", str(sub))
    monkeypatch.setenv("RL_ENV_SPEC", "1")
    task, N, steps = SPECS[sid][1], 8, 12
    desc, extra = load_bundle(task)
    h, to, eo = build_world(desc, extra, N, 0)
    a = NativeEnv(desc, h, to, eo, N, 5, 0, emu_lib)
    b = NativeEnv(desc, h, to, eo, N, 5, 0, allslots_lib)
    assert a.spec_id() == sid and b.spec_id() == sid
    a.reset(); b.reset()
    rng = np.random.default_rng(0)
    touched = 0
    for s in range(steps):
        act = (rng.random((N, a.num_actions), dtype=np.float32) * 2 - 1).astype(np.float32)
        emu_load_state(b, emu_read_state(a))
        a.step(act.ctypes.data); b.step(act.ctypes.data)
        for name in OUTPUTS:
            xa, xb = host_view(a, name), host_view(b, name)
            assert xa.tobytes() == xb.tobytes(), (task, sub, s, name)
        sa, sb = emu_read_state(a), emu_read_state(b)
        for k in STATE_BUFFERS:
            assert sa[k.lower()].tobytes() == sb[k.lower()].tobytes(), (task, sub, s, k)
        touched += int(np.count_nonzero(sa["contact_timers"][..., 1]))  # current_contact time of a body: it touches
    assert touched > 0, "nothing touched the ground in the whole run: the comparison is too quiet"
