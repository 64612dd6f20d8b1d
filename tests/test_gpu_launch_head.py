"""`-m gpu`: the head of the step kernels (csrc/rl_env_kernels.h env_kernel, csrc/env_terms.h step_front).

A step kernel issues the state words whose addresses need only kernel arguments, tile and lane BEFORE the table image is staged, and the
first LOG_PARTS wavefronts of a launch keep the log ring behind a scalar branch on the wavefront's index, with those words in flight.
Two things can go wrong there that no other test looks at:

1. a padding wavefront of a four-wavefront workgroup (it returns behind the staging barrier) issues the early loads too - it must read
   inside the allocation, and the wavefronts beside it must compute what single-wavefront workgroups compute;
2. a step that reset nobody must hand on its predecessor's `extras["log"]` whether the launch has fewer wavefronts than the ring has
   partial rows (LOG_PARTS = 32), exactly as many, or more.

Every case runs A1 Rough on the term-stack interpreter, A1 Rough on its specialised kernel and G1 Rough in the 32-lane mapping, seed 3,
zero actions.  The env count is padded to a multiple of 16, so in the 16- and 32-lane mappings (4 / 2 envs per wavefront) the wavefront
count is a multiple of 4 and the surplus of N = 4, 20 (A1) and 6 (G1) is wavefronts of PADDING ENVS; a padding WAVEFRONT - one beyond
Npad - exists only where a wavefront holds 8 or 16 envs.  The A1 cases therefore also run the 8- and 4-lane mappings (N = 4: 2 / 3
padding wavefronts, N = 20: 0 / 2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RL_TS_CMD_TIME_LEFT, RL_TS_PUSH_TIME_LEFT = 4, 7  # include/rl_env.h rl_task_state_field
A1, G1 = "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0", "RobotLab-Isaac-Velocity-Rough-Unitree-G1-v0"
# (id, task, RL_ENV_SPEC, RL_ENV_SUB)
KERNELS = [("a1-interpreter", A1, "0", "4"), ("a1-spec", A1, "1", "4"), ("g1-32lane", G1, "1", "8")]


def _make(monkeypatch, task, spec, sub, wg, N):
    from robot_lab_amd.env import ManagerBasedRLEnv

    monkeypatch.setenv("RL_ENV_SPEC", spec)
    monkeypatch.setenv("RL_ENV_SUB", sub)
    monkeypatch.setenv("RL_ENV_WG", wg)
    env = ManagerBasedRLEnv(task, num_envs=N, seed=3, device="cuda:0", specialise=False if spec == "0" else None)
    assert (env._native.spec_id() > 0) == (spec != "0"), env.kernel_kind() if hasattr(env, "kernel_kind") else env._native.spec_id()
    assert env._native.envs_per_wavefront() == 16 // int(sub)
    env.reset()
    return env


def _eventful(env):
    """Time-outs due on each of the next three steps, push / command timers about to expire (tests/test_gpu_canary.py _eventful_state at a
    size of a few envs: every kind of event in the first tile AND in the last one)."""
    st = env.read_state()
    N, L = env.num_envs, env.max_episode_length
    ep = np.arange(N) % 7
    ep[0::3] = L - 1 - (np.arange(len(ep[0::3])) % 3)
    ep[[0, 1, 2, N - 1]] = [L - 1, L - 2, L - 3, L - 1]  # a time-out on each of the three steps, in the first tile; one in the last env
    ts = st["task_state"].copy()
    dt = np.float32(env.step_dt)
    ts[1::4, RL_TS_PUSH_TIME_LEFT] = dt * (1 + np.arange(len(ts[1::4])) % 3).astype(np.float32)
    ts[2::5, RL_TS_CMD_TIME_LEFT] = dt * (1 + np.arange(len(ts[2::5])) % 3).astype(np.float32)
    ts[N - 1, RL_TS_PUSH_TIME_LEFT] = dt
    env.load_state({"task_state": ts, "episode_length": ep})


def _trace(env, torch):
    obs, rew, term, tout, _ = env.step(torch.zeros(env.num_envs, env.num_actions, device="cuda:0"))
    return dict(policy=obs["policy"].cpu().numpy().copy(), critic=obs["critic"].cpu().numpy().copy(), reward=rew.cpu().numpy().copy(),
                terms=env.reward_terms().cpu().numpy().copy(), terminated=term.cpu().numpy().copy(), time_out=tout.cpu().numpy().copy(), **env.read_state())


PADDING = [(k, n) for k in KERNELS for n in ((6,) if k[1] == G1 else (4, 20))]
PADDING += [(("a1-interpreter-8lane", A1, "0", "2"), n) for n in (4, 20)] + [(("a1-spec-4lane", A1, "1", "1"), n) for n in (4, 20)]


@pytest.mark.parametrize("kernel,N", PADDING, ids=[f"{k[0]}-{n}" for k, n in PADDING])
def test_four_wavefront_workgroups_with_padding_match_single(kernel, N, monkeypatch):
    """RL_ENV_WG=-4 against single-wavefront workgroups, three eventful steps from the same state: every output and every read_state()
    field bit for bit.  (The two shapes of a kernel are the same arithmetic - csrc/build_info.json lists no pair whose floating-point
    opcode counts differ - so anything short of equal bits is a wrong value.)"""
    import torch

    _, task, spec, sub = kernel
    a = _make(monkeypatch, task, spec, sub, "1", N)
    b = _make(monkeypatch, task, spec, sub, "-4", N)
    _eventful(a)
    b.load_state(a.read_state())
    dones = 0
    for s in range(3):
        ta, tb = _trace(a, torch), _trace(b, torch)
        for k in ta:
            x, y = np.asarray(ta[k]), np.asarray(tb[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (
                f"step {s}: '{k}' differs between single- and four-wavefront workgroups in {int((x != y).sum())} entries "
                f"(first at {np.argwhere(x != y)[0].tolist() if (x != y).any() else 'NaN bits'})")
        dones += int((ta["terminated"] | ta["time_out"]).sum())
    assert dones >= 4  # the forced time-outs happened (_eventful: envs 0, 1, 2 and N - 1)
    a.close()
    b.close()


def _log_bits(extras):
    log = extras["log"]
    return {k: log[k].detach().cpu().numpy().copy().tobytes() for k in list(log.keys())}


@pytest.mark.parametrize("wg", ["1", "-4"])
@pytest.mark.parametrize("N", [4, 64, 132])
@pytest.mark.parametrize("kernel", KERNELS, ids=[k[0] for k in KERNELS])
def test_log_is_inherited_until_the_next_reset(kernel, N, wg, monkeypatch):
    """One forced time-out on step 1; steps 2 and 3 reset nobody and must show step 1's log bit for bit; a second forced time-out on
    step 4 replaces it.  N = 4 / 64 / 132: fewer wavefronts than the ring has partial rows, about as many, more."""
    import torch

    _, task, spec, sub = kernel
    env = _make(monkeypatch, task, spec, sub, wg, N)
    L = env.max_episode_length
    zero = torch.zeros(N, env.num_actions, device="cuda:0")

    def force_time_out(i):
        ep = env.read_state()["episode_length"].copy()
        ep[i] = L - 1
        env.load_state({"episode_length": ep})

    force_time_out(0)
    _, _, term, tout, extras = env.step(zero)
    done = (term | tout).cpu().numpy()
    assert done.sum() == 1 and bool(tout[0]), f"step 1: expected exactly the forced time-out of env 0, got done envs {np.nonzero(done)[0].tolist()}"
    first = _log_bits(extras)
    assert np.frombuffer(first["Episode_Termination/time_out"], np.float32)[0] == 1.0
    for s in (2, 3):
        _, _, term, tout, extras = env.step(zero)
        assert not bool((term | tout).any()), f"step {s}: an env was done under zero actions - the inheritance was not exercised"
        got = _log_bits(extras)
        assert got.keys() == first.keys()
        for k in first:
            assert got[k] == first[k], f"step {s}: '{k}' of the inherited log is {np.frombuffer(got[k], np.float32)}, step 1 logged {np.frombuffer(first[k], np.float32)}"
    force_time_out(1)
    _, _, term, tout, extras = env.step(zero)
    done = (term | tout).cpu().numpy()
    assert done.sum() == 1 and bool(tout[1])
    last = _log_bits(extras)
    assert np.frombuffer(last["Episode_Termination/time_out"], np.float32)[0] == 1.0  # one reset, not two: step 1's count was not carried on
    rewards = [k for k in first if k.startswith("Episode_Reward/")]
    assert any(last[k] != first[k] for k in rewards), "step 4: the log still holds step 1's episode sums"
    env.close()
