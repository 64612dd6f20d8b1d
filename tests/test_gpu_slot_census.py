"""A run-time step-kernel plugin (robot_lab_amd/jit.py) whose sphere-slot census disagrees with the env's tables is refused, GPU tier.

A Spec's kernel does not walk the sphere slots its SLOT_VALID constant leaves empty (csrc/env_spec.h), so a stale plugin - compiled for
a descriptor with fewer collision spheres - would skip a sphere that exists.  `spec_matches` compares the constant with the tables' word:
the plugin with the edited constant is registered (its ABI stamp is right) but never picked, the env runs the interpreter and says so;
the same source unedited is picked.  In a child process: the plugin registry is per process and must not leak into other tests."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, re, subprocess, sys
sys.path.insert(0, %r)
os.environ["RL_ENV_JIT"] = "0"   # nothing is compiled behind the test's back
os.environ["RL_ENV_SPEC"] = "1"
import torch
from robot_lab_amd import capi, jit
from robot_lab_amd.env import ManagerBasedRLEnv
from robot_lab_amd.scene import build_world, load_bundle

task, tmp = "RobotLab-Isaac-Velocity-Rough-Unitree-B2-v0", sys.argv[1]
lib = capi.load_library()
desc, extra = load_bundle(task)
build_world(desc, extra, 16, 0)
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
procs = []
for name, sid, stale in (("Spec_Stale", 4001, True), ("Spec_Fresh", 4002, False)):
    src = jit.spec_source(lib, desc, name, task, sid)
    m = re.search(r"SLOT_VALID = 0x([0-9a-f]+)u;", src)
    word = int(m.group(1), 16)
    assert word != 0
    if stale:  # the census of a descriptor that lacked one of the spheres: the lowest filled slot cleared
        src = src.replace(m.group(0), "SLOT_VALID = 0x%%xu;" %% (word & (word - 1)))
    path = os.path.join(tmp, name + ".hip")
    open(path, "w").write(jit.plugin_source(src, name, sid))
    out = os.path.join(tmp, name + ".so")
    procs.append((out, subprocess.Popen([hipcc, *jit.ENV_FLAGS, jit.stamp_flag(), "-DRL_ENV_SPEC_SUB=4", "-shared", "-fPIC", "-o", out, path])))
for out, p in procs:
    assert p.wait() == 0, out
stale_so, fresh_so = procs[0][0], procs[1][0]

def run():
    env = ManagerBasedRLEnv(task, num_envs=64, seed=3, device="cuda:0")
    env.reset()
    env.step(torch.zeros(64, env.num_actions, device="cuda:0"))
    torch.cuda.synchronize()
    got = (env._native.spec_id(), env.step_kernel)
    env.close()
    return got

n0 = lib.rl_env_spec_plugin_count()
assert lib.rl_env_register_spec_plugin(stale_so.encode()) == 0, lib.rl_env_last_error()
assert lib.rl_env_spec_plugin_count() == n0 + 1
sid, kernel = run()
assert sid == 0 and kernel == "interpreter", (sid, kernel)
assert lib.rl_env_register_spec_plugin(fresh_so.encode()) == 0, lib.rl_env_last_error()
sid, kernel = run()
assert sid == 4002 and kernel == "specialised (spec_id 4002)", (sid, kernel)
print("CENSUS_PLUGIN_OK")
''' % ROOT


@pytest.mark.gpu
def test_plugin_with_a_stale_slot_census_is_refused(tmp_path):
    p = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CENSUS_PLUGIN_OK" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
