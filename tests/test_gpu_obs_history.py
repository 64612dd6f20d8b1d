"""`-m gpu`: observation history (include/rl_env.h rl_env_set_obs_history) on the HIP library - the history kernel
(csrc/rl_env_history.hip) against the numpy restatement of the contract, inside a captured collection loop, and under both learners."""
import numpy as np
import pytest

from test_obs_history import HistoryRule

pytestmark = pytest.mark.gpu

A1F = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
G1F = "RobotLab-Isaac-Velocity-Flat-Unitree-G1-v0"


def _lists(desc):
    pol = [(3, 0, 1, 2)[i % 4] for i in range(desc.task.n_policy)]
    cri = [2] * desc.task.n_critic
    cri[1] = 0
    return {"policy": pol, "critic": cri}


@pytest.mark.parametrize("task,N", [(A1F, 37), (G1F, 5)])  # N is no multiple of the envs per wavefront: Npad > N
def test_history_rows_are_bit_exact(task, N):
    import torch

    from robot_lab_amd import shims

    shims.install()  # gymnasium (or its shim): the env then carries observation spaces
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.scene import load_bundle

    desc, _ = load_bundle(task)
    hist = _lists(desc)
    A = ManagerBasedRLEnv(task, num_envs=N, seed=5, device="cuda:0")
    B = ManagerBasedRLEnv(task, num_envs=N, seed=5, device="cuda:0", obs_history=hist)
    assert A.obs_history == {} and B.obs_history == hist and "obs_history" in repr(B) and "obs_history" not in repr(A)
    rules = {n: HistoryRule(desc.obs_term_dims(g), hist[n], N) for g, n in enumerate(("policy", "critic"))}
    for n in rules:
        assert B.single_observation_space[n].shape == (rules[n].row.shape[1],) and B.observation_space[n].shape == (N, rules[n].row.shape[1])
    ring = B._bufs["OBS_POLICY_RING"]
    assert ring.shape[1] > N and ring.shape[2] == rules["policy"].row.shape[1]

    def check(oa, ob, reset, what):
        torch.cuda.synchronize()
        for n in ("policy", "critic"):
            frame = oa[n].cpu().numpy()
            want = rules[n].push(frame, reset)
            got = ob[n].cpu().numpy()
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {n} history row differs from the rule"
        for n in ("OBS_POLICY_RING", "OBS_CRITIC_RING"):
            assert not bool(B._bufs[n][:, N:].any()), f"{what}: rows at and above N of {n} were written"

    def frames_equal(what):
        fa, fb = A.get_observation_frames(), B.get_observation_frames()
        for n in ("policy", "critic"):
            assert fa[n].data_ptr() == A.get_observations()[n].data_ptr()  # no history: the frame IS the row
            assert torch.equal(fb[n], A.get_observations()[n]), f"{what}: the {n} frame of the history env differs from the plain env's row"

    oa, _ = A.reset()
    ob, _ = B.reset()
    check(oa, ob, np.ones(N, dtype=bool), "reset()")
    frames_equal("reset()")
    L = A.max_episode_length
    ep = torch.zeros(N, dtype=torch.int64)
    ep[3], ep[2] = L - 3, L - 7  # time out in steps 2 and 6
    for e in (A, B):
        e.episode_length_buf = ep
    zero = torch.zeros(N, A.num_actions, device="cuda:0")
    ever, late = np.zeros(N, dtype=bool), False
    for step in range(8):
        oa, _, ta, oa_to, _ = A.step(zero)
        ob, _, tb, ob_to, _ = B.step(zero)
        done = (ta | oa_to).cpu().numpy()
        assert np.array_equal(done, (tb | ob_to).cpu().numpy())
        ever |= done
        late = late or (step >= 2 and done.any())
        check(oa, ob, done, f"step {step}")
        frames_equal(f"step {step}")
        if step == 3:
            ids = [1, N - 1]
            oa, _ = A.reset(env_ids=ids)
            ob, _ = B.reset(env_ids=ids)
            mask = np.zeros(N, dtype=bool)
            mask[ids] = True
            check(oa, ob, mask, "reset(env_ids)")
    assert late and not ever.all()
    # read_state / load_state carry the current slot
    st = B.read_state()
    assert st["obs_history_policy"].shape == rules["policy"].row.shape and np.array_equal(st["obs_history_policy"], rules["policy"].row)
    assert "obs_history_policy" not in A.read_state()
    saved = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in st.items()}
    B.step(zero)
    B.load_state(saved)
    torch.cuda.synchronize()
    assert np.array_equal(B.get_observations()["policy"].cpu().numpy(), saved["obs_history_policy"])
    A.close(); B.close()


def _collector(use_graph, N=64, T=4, hist=3):
    import torch

    from robot_lab_amd.collect import Collector
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.rollout import RolloutStorage

    from robot_lab_amd.scene import load_bundle

    critic = [(0, 2, 0, 1)[i % 4] for i in range(load_bundle(A1F)[0].task.n_critic)]
    env = ManagerBasedRLEnv(A1F, num_envs=N, seed=11, device="cuda:0", obs_history={"policy": hist, "critic": critic})
    obs, _ = env.reset()
    ep = torch.arange(N) % 9
    ep[::5] = env.max_episode_length - 1 - (torch.arange(len(ep[::5])) % 6)  # time-out resets inside every collection
    env.episode_length_buf = ep
    od, cd, A = obs["policy"].shape[1], obs["critic"].shape[1], env.num_actions
    rng = np.random.default_rng(0)

    def net(dims):
        ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
        return MlpPolicy(ws, [0.05 * rng.standard_normal(d).astype(np.float32) for d in dims[1:]], "elu", device="cuda:0")

    actor, critic = net([od, 512, 256, 128, A]), net([cd, 512, 256, 128, 1])
    storage = RolloutStorage(N, T, od, cd, A, seed=3, device="cuda:0")
    std = torch.full((A,), 0.5, device="cuda:0")
    return env, storage, Collector(env, actor, critic, storage, std, use_graph=use_graph)


def test_captured_collection_equals_the_eager_one():
    """T = 4 steps per collection: iteration 0 of the graphed collector is eager + capture, 1 and 2 are replays."""
    import torch

    env_e, st_e, eager = _collector(False)
    env_g, st_g, graph = _collector(True)
    assert st_e.observations.shape[-1] == 135
    dones = 0
    for it in range(3):
        oe, og = eager.collect(), graph.collect()
        torch.cuda.synchronize()
        for name in ("observations", "privileged_observations", "actions", "mu", "actions_log_prob", "values", "rewards", "dones", "returns", "advantages"):
            a, b = getattr(st_e, name), getattr(st_g, name)
            assert torch.equal(a, b), f"iteration {it}: {name} differs (max |d| {float((a.float() - b.float()).abs().max()):.3e})"
        assert torch.equal(oe["policy"], og["policy"]) and torch.equal(oe["critic"], og["critic"])
        dones += int(st_g.dones.sum())
        # the stored rows ARE history rows: slot t's newest policy frame is slot t + 1's middle frame for envs step t did not reset
        obs, done = st_g.observations, st_g.dones.reshape(st_g.dones.shape[0], -1).bool()
        for t in range(obs.shape[0] - 1):
            keep = ~done[t]
            assert torch.equal(obs[t + 1][keep][:, 3:6], obs[t][keep][:, 6:9])  # term 0 (3 wide, H = 3): slots [0:3 | 3:6 | 6:9]
    assert dones > 0
    env_e.close(); env_g.close()


@pytest.mark.parametrize("learner", ["torch", "hip"])
@pytest.mark.parametrize("symmetry", [None, "lr"])
def test_training_on_a_history_env(learner, symmetry):
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1F, num_envs=64, seed=3, device="cuda:0", obs_history={"policy": 3})
    tr = Trainer(env, num_steps_per_env=4, seed=3, learner=learner, symmetry=symmetry)
    assert tr.policy.actor[0].in_features == 135 and tr.storage.observations.shape[-1] == 135
    if symmetry:
        assert tr.symmetry.obs[0].shape[1] == 135
    row = env.get_observations()["policy"].clone()  # what the first collection step sees
    for it in range(2):
        out = tr.iterate()
        torch.cuda.synchronize()
        assert np.isfinite(float(out["surrogate_loss"])) and np.isfinite(float(out["value_loss"])) and np.isfinite(out["mean_reward"])
        if it == 0:  # the storage's observation slot is the env's row
            assert torch.equal(tr.storage.observations[0].reshape(64, 135), row)
    env.close()


def test_a_row_wider_than_the_kernels_take_is_refused():
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.ppo import Trainer

    env = ManagerBasedRLEnv(A1F, num_envs=16, seed=3, device="cuda:0", obs_history={"policy": 12})  # 45 x 12 = 540 > 512
    assert env.get_observations()["policy"].shape == (16, 540)  # the env itself takes any width
    with pytest.raises(ValueError, match=r"policy observation row is 540 columns wide.*at most 512"):
        Trainer(env, num_steps_per_env=4)
    env.close()
