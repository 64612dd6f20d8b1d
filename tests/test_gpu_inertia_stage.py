"""`-m gpu`: the staged rigid-body records of the quadruped step kernels (robot_lab_amd/csrc/env_step.h LsFor::INERTIA_STAGE).

With 16 lanes per env every lane reads the rigid-body words of its link(s) and of the base link once per launch into its LDS scratchpad and
the four substeps take them from there.  The start-up randomisation gives every env its own masses and centres of mass, so a record staged
from another env, limb or link - or a granule of another lane - moves the step away from the fp64 oracle by far more than round-off:
  * A1 Rough on its specialised kernel, A1 Rough on the interpreter's kernel, Go2W Rough (the merged four-joint instance);
  * 6 envs (a partial tile) and 64 envs in single-wavefront workgroups, 64 envs in four-wavefront workgroups (RL_ENV_WG=-4: 16 tiles in four
    workgroups, and at 6 envs nothing but a padding tile would remain, so that shape runs at 64);
  * two steps from reset(): the second one is held to the oracle from the shared state with the per-env bound and the flat ceilings of
    helpers.teacher_forced_check / HARD_CAPS (at most three envs on a switch, as tests/test_gpu_parity.py allows at these sizes), and the two
    workgroup shapes must agree bit for bit in everything they return and carry.
The state exchange (rl_env_export_state / rl_env_commit_state) carries no rigid-body words - they are written by the host at start-up only -,
so there is no case that changes them between two steps."""
import numpy as np
import pytest

from helpers import HARD_CAPS, teacher_forced_check
from oracle.env import OracleEnv
from robot_lab_amd.scene import build_world, load_bundle

pytestmark = pytest.mark.gpu

A1 = "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0"
GO2W = "RobotLab-Isaac-Velocity-Rough-Unitree-Go2W-v0"
CASES = [(A1, True), (A1, False), (GO2W, True)]  # (task, specialised kernel)


def _two_steps(task, N, wg, seed=7):
    """reset + two steps; returns (state before the second step, its action, everything after it, spec id)"""
    import os

    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv

    os.environ["RL_ENV_WG"] = wg
    try:
        env = ManagerBasedRLEnv(task, num_envs=N, seed=seed, device="cuda:0")
    finally:
        del os.environ["RL_ENV_WG"]
    assert env._native.envs_per_wavefront() == 4
    env.reset()
    g = torch.Generator().manual_seed(13)
    acts = [(torch.rand(N, env.num_actions, generator=g) * 2 - 1) for _ in range(2)]
    env.step(acts[0].cuda())
    state = env.read_state()
    obs, rew, term, tout, _ = env.step(acts[1].cuda())
    got = env.read_state()
    got.update(reward=rew.cpu().numpy(), reward_terms=env.reward_terms().cpu().numpy(), done=(term | tout).cpu().numpy(),
               obs_policy=obs["policy"].cpu().numpy(), obs_critic=obs["critic"].cpu().numpy())
    sid = env._native.spec_id()
    env.close()
    return state, acts[1].numpy(), got, sid


@pytest.mark.parametrize("task,spec", CASES)
def test_two_steps_from_reset_against_the_oracle_and_across_workgroup_shapes(task, spec, monkeypatch):
    monkeypatch.delenv("RL_ENV_WG", raising=False)
    monkeypatch.setenv("RL_ENV_SUB", "4")
    monkeypatch.setenv("RL_ENV_SPEC", "1" if spec else "0")
    runs = {(N, wg): _two_steps(task, N, wg) for N, wg in ((6, "1"), (64, "1"), (64, "-4"))}
    for (N, wg), (state, a, got, sid) in runs.items():
        assert (sid > 0) == spec, (N, wg, sid)
    # the two workgroup shapes: same arithmetic on the same words
    (s1, a1, g1, _), (s4, a4, g4, _) = runs[(64, "1")], runs[(64, "-4")]
    for k in s1:
        assert np.array_equal(s1[k], s4[k]), ("state before the second step", k)
    for k in g1:
        assert np.array_equal(g1[k], g4[k]), ("after the second step", k)
    # against the oracle, one step from the shared state (the four-wavefront run is the single-wavefront one bit for bit)
    desc, extra = load_bundle(task)
    for N in (6, 64):
        state, a, got, _ = runs[(N, "1")]
        h, to, eo = build_world(desc, extra, N, 0)
        ora = OracleEnv(desc, h, to, N, 7, eo)
        rep = teacher_forced_check(ora, state, a, got, n_twins=6, max_mask=3.0 / N, caps=HARD_CAPS)
        print(f"\n[inertia-stage] {task} spec={spec} N={N}: masked {rep['masked']}/{N}, root {rep['root_state']['max_err']:.2e}, "
              f"qd {rep['joint_vel']['max_err']:.2e}, critic {rep['obs_critic']['max_err']:.2e}")
