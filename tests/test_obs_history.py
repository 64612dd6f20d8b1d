"""Observation history (include/rl_env.h rl_env_set_obs_history) on the CPU lane emulator, whose host loop runs the same per-element
rule (csrc/env_history.h history_element) the HIP kernel runs: an env WITH history must show, bit for bit, a numpy restatement of the
contract applied to the frames and reset flags of an env WITHOUT history on the same seed."""
import numpy as np
import pytest

from helpers import emu_load_state, emu_read_state, host_view
from robot_lab_amd import capi
from robot_lab_amd.scene import build_world, load_bundle

TASK, N, SEED = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0", 16, 5
POLICY_H = [3, 0, 1, 3, 2, 0]  # per term: the lengths differ between terms and include 0, 1 and 3
GROUPS = ("POLICY", "CRITIC")


def critic_h(desc):
    h = [2] * desc.task.n_critic
    h[1] = 0
    return h


def make(emu_lib, hist=None):
    desc, extra = load_bundle(TASK)
    h, to, eo = build_world(desc, extra, N, 0)
    return desc, capi.NativeEnv(desc, h, to, eo, N, SEED, 0, emu_lib, obs_history=hist)


class HistoryRule:
    """numpy restatement of the contract: term k (width d_k, length H_k) owns max(H_k, 1) frames of its block, oldest first; a push
    moves every slot one frame towards the old end and appends the frame; an env reset by the launch has every slot = the frame."""

    def __init__(self, dims, hist, n):
        self.dims, self.hist = list(dims), [max(1, h) for h in hist]
        self.row = np.zeros((n, sum(d * h for d, h in zip(self.dims, self.hist))), dtype=np.float32)  # the ring starts zeroed

    def push(self, frame, reset):
        new, off, foff = np.empty_like(self.row), 0, 0
        for d, H in zip(self.dims, self.hist):
            f = frame[:, foff:foff + d]
            for s in range(H):
                kept = f if s == H - 1 else self.row[:, off + (s + 1) * d: off + (s + 2) * d]
                new[:, off + s * d: off + (s + 1) * d] = np.where(reset[:, None], f, kept)
            off, foff = off + H * d, foff + d
        self.row = new
        return self.row


@pytest.fixture()
def sub1(monkeypatch):
    monkeypatch.setenv("RL_EMU_SUB", "1")  # one lane per limb: the fast mapping of the emulator


def test_history_rows_follow_the_rule(emu_lib, sub1):
    desc, A = make(emu_lib)
    hist = {"policy": POLICY_H, "critic": critic_h(desc)}
    assert len(POLICY_H) == desc.task.n_policy and {0, 1, 3} <= set(POLICY_H) and 2 in hist["critic"]
    _, B = make(emu_lib, hist)
    assert [B.obs_history(g) for g in (0, 1)] == [hist["policy"], hist["critic"]] and A.obs_history(0) == [0] * desc.task.n_policy
    rules = [HistoryRule(desc.obs_term_dims(g), hist[n], N) for g, n in enumerate(("policy", "critic"))]
    assert [B.obs_dim(g) for g in (0, 1)] == [r.row.shape[1] for r in rules] == [desc.obs_dim(g, hist[n]) for g, n in enumerate(("policy", "critic"))]
    assert [A.obs_dim(g) for g in (0, 1)] == [desc.obs_dim(0), desc.obs_dim(1)]

    def check(reset, what):
        for g, name in enumerate(GROUPS):
            frame = host_view(A, "OBS_" + name).copy()
            assert host_view(B, f"OBS_{name}_FRAME").shape == frame.shape
            assert np.array_equal(host_view(B, f"OBS_{name}_FRAME"), frame), f"{what}: {name} frame of the history env differs from the plain env's row"
            want = rules[g].push(frame, reset)
            got = host_view(B, "OBS_" + name)
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {name} history row differs from the rule"
            ring = host_view(B, f"OBS_{name}_RING")
            assert np.array_equal(ring[B.obs_slot(), :N], got) and not ring[:, N:].any()  # rows N..Npad are never written

    for e in (A, B):
        e.reset()
    check(np.ones(N, dtype=bool), "reset()")
    L = A.max_episode_length
    for e in (A, B):  # named envs time out at named steps
        ep = host_view(e, "EPISODE_LENGTH")
        ep[:] = 0
        ep[3], ep[7], ep[11] = L - 2, L - 4, L - 6
    zero = np.zeros((N, A.num_actions), dtype=np.float32)
    ever, late, partial = np.zeros(N, dtype=bool), False, False
    for step in range(8):
        for e in (A, B):
            e.step(zero.ctypes.data)
        done = (host_view(A, "TERMINATED") | host_view(A, "TIME_OUT")).astype(bool)
        assert np.array_equal(done, (host_view(B, "TERMINATED") | host_view(B, "TIME_OUT")).astype(bool))
        ever |= done
        late = late or (step >= 2 and done.any())
        check(done, f"step {step}")
        if step == 3:  # a partial reset in the middle: the listed envs are filled, every other env pushes one frame
            ids = [1, 5, 11]
            for e in (A, B):
                e.reset(ids)
            mask = np.zeros(N, dtype=bool)
            mask[ids] = True
            check(mask, "reset(env_ids)")
            partial = True
    # required coverage (preconditions of the comparison above, not skips)
    assert late, "no env was reset by a step at or after step 2"
    assert not ever.all() and not ever[0], "every env was reset by some step: no row ever held frames of different steps for its whole length"
    assert partial
    A.close(); B.close()


def test_all_zero_lists_change_nothing(emu_lib, sub1):
    desc, A = make(emu_lib)
    _, Z = make(emu_lib)
    before = {n: Z.buffer(n)[0] for n in ("OBS_POLICY", "OBS_CRITIC", "OBS_POLICY_RING", "OBS_CRITIC_RING")}
    Z.set_obs_history(0, [0] * desc.task.n_policy)
    Z.set_obs_history(1, [0] * desc.task.n_critic)
    assert {n: Z.buffer(n)[0] for n in before} == before
    zero = np.zeros((N, A.num_actions), dtype=np.float32)
    for e in (A, Z):
        e.reset()
        e.step(zero.ctypes.data)
        e.step(zero.ctypes.data)
    for name in GROUPS:
        assert Z.buffer(f"OBS_{name}_FRAME")[:2] == Z.buffer("OBS_" + name)[:2]  # no history: the frame IS the row
        assert Z.buffer("OBS_" + name)[1] == A.buffer("OBS_" + name)[1]
        assert np.array_equal(host_view(Z, "OBS_" + name).view(np.uint32), host_view(A, "OBS_" + name).view(np.uint32))
    A.close(); Z.close()


def test_refusals_carry_their_reason(emu_lib, sub1):
    desc, E = make(emu_lib)
    n = desc.task.n_policy
    with pytest.raises(capi.RlEnvError, match="outside 0..32"):
        E.set_obs_history(0, [33] + [0] * (n - 1))
    with pytest.raises(capi.RlEnvError, match="outside 0..32"):
        E.set_obs_history(0, [-1] + [0] * (n - 1))
    with pytest.raises(capi.RlEnvError, match=f"lengths for a group of {n} terms"):
        E.set_obs_history(0, [1] * (n + 1))
    with pytest.raises(capi.RlEnvError, match="group must be"):
        E.set_obs_history(2, [1] * n)
    E.set_obs_history(0, [2] * n)  # (the refused calls above did not use up the group's one call)
    with pytest.raises(capi.RlEnvError, match="already set"):
        E.set_obs_history(0, [2] * n)
    E.reset()
    E.step(np.zeros((N, E.num_actions), dtype=np.float32).ctypes.data)
    with pytest.raises(capi.RlEnvError, match="after the first rl_env_reset / rl_env_step"):
        E.set_obs_history(1, [1] * desc.task.n_critic)
    assert E.obs_history(0) == [2] * n and E.obs_history(1) == [0] * desc.task.n_critic
    E.close()


def test_history_survives_a_state_round_trip(emu_lib, sub1):
    """History is carried state: what the Python boundary's read_state() / load_state() do - the current slot out, and back into the current
    slot of another env - makes the next step shift the SAVED frames."""
    desc, B = make(emu_lib, {"policy": POLICY_H})
    _, C = make(emu_lib, {"policy": POLICY_H})
    zero = np.zeros((N, B.num_actions), dtype=np.float32)
    B.reset()
    for _ in range(3):
        B.step(zero.ctypes.data)
    state = emu_read_state(B)
    saved = host_view(B, "OBS_POLICY").copy()  # read_state()["obs_history_policy"]
    C.reset()  # (C sits in the other ring slot than B: "current slot" is what is saved and loaded)
    assert C.obs_slot() != B.obs_slot()
    emu_load_state(C, state)
    host_view(C, "OBS_POLICY")[...] = saved  # load_state()
    C.step(zero.ctypes.data)
    keep = ~(host_view(C, "TERMINATED") | host_view(C, "TIME_OUT")).astype(bool)
    assert keep.sum() >= N // 2
    row, frame, off, foff = host_view(C, "OBS_POLICY"), host_view(C, "OBS_POLICY_FRAME"), 0, 0
    for d, h in zip(desc.obs_term_dims(0), POLICY_H):
        H = max(1, h)
        # the H - 1 older slots are the saved row's H - 1 newest slots, exactly; the newest slot is the step's frame
        assert np.array_equal(row[keep, off:off + (H - 1) * d].view(np.uint32), saved[keep, off + d:off + H * d].view(np.uint32))
        assert np.array_equal(row[:, off + (H - 1) * d:off + H * d], frame[:, foff:foff + d])
        off, foff = off + H * d, foff + d
    B.close(); C.close()
