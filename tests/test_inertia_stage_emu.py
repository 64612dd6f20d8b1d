"""The staged rigid-body records of the quadruped step (robot_lab_amd/csrc/env_step.h LsFor::INERTIA_STAGE, EnvLane::stage_inertia_*), CPU tier.

With 16 lanes per env a quadruped lane reads the rigid-body words of its link(s) and of the base link ONCE per step into its scratchpad and
takes them from there in every substep; -DRL_INERTIA_RELOAD compiles the form that reads them from the state tiles in every substep.  The two
are the same arithmetic on the same words, so the lane emulator built one way and the other (a second build, ~2 minutes of g++, once per
session) must give the same bits: every output and every state buffer, step by step, on A1 Rough (three-joint limbs, a base link group) and
Go2W Rough (the merged four-joint instance) at 6 envs - a partial tile.  The start-up randomisation gives every env its own masses and centres
of mass, so a record staged from another env, limb or link changes the words."""
import os
import subprocess

import numpy as np
import pytest

from helpers import STATE_BUFFERS, emu_read_state, host_view
from robot_lab_amd.capi import NativeEnv
from robot_lab_amd.scene import build_world, load_bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("OBS_POLICY", "OBS_CRITIC", "REWARD", "REWARD_TERMS", "TERMINATED", "TIME_OUT")
TASKS = ("RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0", "RobotLab-Isaac-Velocity-Rough-Unitree-Go2W-v0")


@pytest.fixture(scope="session")
def reload_lib(tmp_path_factory, emu_lib):
    out = str(tmp_path_factory.mktemp("emu_inertia_reload") / "librl_env_emu_inertia_reload.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-shared", "-fPIC", "-DRL_INERTIA_RELOAD", "-o", out,
                    os.path.join(ROOT, "tests", "emu", "rl_env_emu.cpp")], check=True)
    return out


@pytest.mark.parametrize("spec", [1, 0])  # the task's specialised program, the interpreter
@pytest.mark.parametrize("task", TASKS)
def test_staged_records_equal_reloaded_records_bit_for_bit(task, spec, emu_lib, reload_lib, monkeypatch):
    monkeypatch.setenv("RL_EMU_FIBERS", "1")
    monkeypatch.setenv("RL_EMU_SUB", "4")  # 16 lanes per env: the mapping that stages
    monkeypatch.setenv("RL_ENV_SPEC", str(spec))
    N, steps = 6, 8
    desc, extra = load_bundle(task)
    h, to, eo = build_world(desc, extra, N, 0)
    a = NativeEnv(desc, h, to, eo, N, 5, 0, emu_lib)
    b = NativeEnv(desc, h, to, eo, N, 5, 0, reload_lib)
    assert (a.spec_id() != 0) == bool(spec) and a.spec_id() == b.spec_id()
    assert a.envs_per_wavefront() == b.envs_per_wavefront() == 4
    a.reset(); b.reset()
    rng = np.random.default_rng(0)
    for s in range(steps):
        act = (rng.random((N, a.num_actions), dtype=np.float32) * 2 - 1).astype(np.float32)
        a.step(act.ctypes.data); b.step(act.ctypes.data)
        for name in OUTPUTS:
            assert host_view(a, name).tobytes() == host_view(b, name).tobytes(), (task, spec, s, name)
        sa, sb = emu_read_state(a), emu_read_state(b)
        for k in STATE_BUFFERS:
            assert sa[k.lower()].tobytes() == sb[k.lower()].tobytes(), (task, spec, s, k)
    assert np.isfinite(host_view(a, "OBS_POLICY")).all() and np.unique(host_view(a, "REWARD")).size > 1  # the envs moved, each its own way
