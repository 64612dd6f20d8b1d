"""`-m gpu`: the off-the-platform parity checks (tests/terrain_helpers.py; CPU tier: tests/test_terrain_contacts.py) on the HIP library, driven
through the C-ABI with a heightfield of the test's own: robots placed over the hash-coded field, on the waves, mid-slope, across stair
risers, tile seams and the grid's edges, ONE teacher-forced step against the fp64 oracle - helpers.teacher_forced_check and the contact
forces (a), the height-scan lookup alone on the kernel's own post-step state (b), the family's claims (c) - in every kernel shape
tests/test_gpu_parity.py forces.  Neither the custom field nor term_out_of_bounds = 0 changes which kernel runs (spec_matches looks at
neither): A1 Rough runs its Spec.  Plus the GPU twin of the two moved envs of tests/test_teacher_forced.py."""
import os

import numpy as np
import pytest

import terrain_helpers as th

pytestmark = pytest.mark.gpu

# (task, shape name, environment, envs): A1's Spec kernel and the interpreter, the four-wavefront workgroup, one and two sub-lanes per limb; Go2W
# (wheels, the merged instance); G1 in the 16- and the 32-lane mapping; Tita (base_height_l2 with its 3 x 3 ray caster, on the interpreter)
SHAPES = [
    (th.A1, "spec", {}, 64), (th.A1, "interp", {"RL_ENV_SPEC": "0"}, 64), (th.A1, "wg-4", {"RL_ENV_WG": "-4"}, 64),
    (th.A1, "sub1", {"RL_ENV_SUB": "1"}, 64), (th.A1, "sub2", {"RL_ENV_SUB": "2"}, 64),
    (th.GO2W, "default", {}, 64),
    (th.G1, "sub4", {"RL_ENV_SUB": "4"}, 32), (th.G1, "sub8", {"RL_ENV_SUB": "8"}, 32),
    (th.TITA, "default", {}, 64),
]


@pytest.mark.parametrize("family", list(th.FAMILIES))
@pytest.mark.parametrize("task,shape,env,N", SHAPES, ids=[f"{t.split('-')[-2]}-{s}" for t, s, _, _ in SHAPES])
def test_placed_robots_match_the_oracle(task, shape, env, N, family, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    field, _, mutate, _ = th.FAMILIES[family]
    desc, h, to = th.make_world(task, N, field, mutate)
    drv = th.Driver(desc, h, to, N, 42, gpu=True)
    if task == th.A1:
        assert (drv.nat.spec_id() != 0) == (shape != "interp"), drv.nat.spec_id()  # the production Spec kernel, custom field or not
    if "RL_ENV_SUB" in env:
        assert drv.nat.envs_per_wavefront() == 16 // int(env["RL_ENV_SUB"])
    ora = th.oracle_for(desc, h, to, N, 42)
    rep = th.run_case(family, drv, ora, key=task)
    line = th.profile_line(task, shape, rep)
    print("\n[terrain-parity]", line, rep.get("claims"))
    out_dir = os.environ.get("RL_REPORT_DIR", "")
    if out_dir and os.path.isdir(out_dir):  # the measured ratios of check (b) of an analysis run: profiles/terrain_parity.txt is such a file
        with open(os.path.join(out_dir, "terrain_parity.txt"), "a") as f:
            f.write(line + "\n")
    drv.close()


def test_moved_envs_level_up_and_out_of_bounds():
    """The GPU twin of the two moved envs of tests/test_teacher_forced.py: one env 4.5 m off its origin on the step its episode times out -
    terrain_levels_vel moves it one level up (velocity_env_cfg.py:671); one past 0.5 x width - oob_buffer - terrain_out_of_bounds
    (:656-664), a time-out-type termination: TIME_OUT is set, TERMINATED is not, and the episode log counts it."""
    import torch

    from oracle.physics import TerrainSampler
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.scene import build_world, load_bundle

    N, up, oob = 64, 1, 6
    env = ManagerBasedRLEnv(th.A1, num_envs=N, seed=42, device="cuda:0")
    desc, extra = load_bundle(th.A1)
    h, _, _ = build_world(desc, extra, N, 0)
    td, tk = desc.terrain, desc.task
    assert tk.term_out_of_bounds and td.curriculum
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    for _ in range(2):
        env.step(torch.rand(N, env.num_actions, device="cuda", generator=g) * 2 - 1)
    state = env.read_state()
    rs = state["root_state"].copy()
    rs[up, 0] += 4.5
    rs[oob, 0] = 0.5 * (td.num_rows * td.tile_size + 2 * td.border) - tk.oob_buffer + 0.5
    ground = TerrainSampler(td, h)
    for i in (up, oob):
        rs[i, 2] = ground.sample(rs[i, 0:1].astype(np.float64), rs[i, 1:2].astype(np.float64))[0][0] + 0.45
        rs[i, 3:7] = [1.0, 0.0, 0.0, 0.0]
        rs[i, 7:13] = 0.0
    state["root_state"] = rs
    ep = state["episode_length"].copy()
    ep[:] = 5
    ep[up] = env.max_episode_length - 1  # times out on the compared step
    state["episode_length"] = ep
    level_before = state["terrain_level"].copy()
    assert level_before[up] < td.num_rows - 1
    env.load_state(state)
    _, _, term, tout, extras = env.step(torch.rand(N, env.num_actions, device="cuda", generator=g) * 2 - 1)
    term, tout = term.cpu().numpy(), tout.cpu().numpy()
    assert tout[up] and tout[oob] and not term[oob] and not term[up]
    assert (term | tout).sum() == 2  # nobody else was reset: the log below is theirs
    after = env.read_state()
    assert after["terrain_level"][up] == level_before[up] + 1
    assert after["episode_length"][up] == 0 and after["episode_length"][oob] == 0
    log = extras["log"]
    assert float(log["Episode_Termination/terrain_out_of_bounds"]) == 1.0 and float(log["Episode_Termination/time_out"]) == 1.0
    env.close()
