"""`-m gpu`: what a specialised step kernel (robot_lab_amd/csrc/env_spec.h) does behind its last substep - time-out reset, push, both
observation rows, the noise pass - on the quadruped Specs with several sub-lanes per limb, at launch sizes of one partly filled wavefront
(1 env), a full one plus a partial one (5) and more wavefronts than a workgroup holds with a padding wavefront (68):

  (a) one step of the Spec's kernel and of the interpreter's kernel of the same library from a shared state, twice: a step in which env 0
      times out, and a step with the push interval forced due in every env.  Observation rows within the bound tests/test_gpu_specs.py
      applies to them (the figures stand inline in its test body, so they are restated here, not imported): every entry within 2e-3
      relative to max(|interpreter|, 1), the 99th percentile within 2e-5;
  (b) the noise of the policy row inside ONE kernel: two Spec envs from the same state and seed, corruption on and off.  For every column
      whose clip binds in neither, noisy / scale - clean / scale = noise_lo + (noise_hi - noise_lo) u to 1 ulp (fp32) of the largest
      operand of that identity - the two values and the draw: the kernel rounds the draw and the sum once each, half an ulp of its own
      result either time, and a draw that nearly cancels the value is the largest of the three -, u from oracle/philox.py at (seed, env,
      step, noise stream, column >> 2), component column & 3.  `x / scale` is taken as what it stands for - an fp32 value whose product
      with the fp32 scale rounds to x: for a scale that is no power of two (joint velocities, 0.05) the quotient in floating point carries the product's rounding twice, up to 2 ulp that no kernel could avoid (measured on the
      CPU lane emulator with the plain quotient: 1.6 ulp in those columns, <= 1 in all others);
  (c) the play variant (corruption switched off at run time on a Spec that corrupts): the policy row equals, bit for bit, the critic's columns
      of the same term wherever the two groups give the term the same clip and scale; the other terms are named in the printed line."""
import json

import numpy as np
import pytest

from oracle import philox as px

pytestmark = pytest.mark.gpu

TASKS = {
    1: "RobotLab-Isaac-Velocity-Rough-Unitree-A1-v0",   # 45 / 235 columns: 45 = 11 four-column blocks + 1 column
    5: "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0",    # 45 / 48, no height scan
    3: "RobotLab-Isaac-Velocity-Rough-Unitree-Go2W-v0",  # 57 / 247, wheel columns
}
CASES = [(sid, sub, n) for sid in (1, 5, 3) for sub in ("4", "2") for n in (1, 5, 68)]
SEED = 11
OBS_MAX, OBS_P99 = 2e-3, 2e-5  # tests/test_gpu_specs.py: worst["obs"], worst["obs_p99"]
RL_TS_PUSH_TIME_LEFT = 7       # include/rl_env.h
KIND_NAMES = ("base_lin_vel", "base_ang_vel", "projected_gravity", "velocity_commands", "joint_pos_rel", "joint_vel_rel", "last_action", "height_scan",
              "joint_pos_rel_no_wheel")


def term_columns(task_desc, group, n_joints):
    """[(term index, kind, first column, width)] of an observation group, in row order"""
    terms, n = (task_desc.policy, task_desc.n_policy) if group == "policy" else (task_desc.critic, task_desc.n_critic)
    out, off = [], 0
    for i in range(n):
        k = int(terms[i].kind)
        w = 3 if k <= 3 else (int(task_desc.scan_nx) * int(task_desc.scan_ny) if k == 7 else n_joints)
        out.append((i, k, off, w))
        off += w
    return out


def preimages(y, scale):
    """The fp32 values x with fl32(x * scale) == y, as (candidates [5, ...], valid mask): the two neighbours each side of fl32(y / scale)."""
    y = np.asarray(y, dtype=np.float32)
    x0 = (y.astype(np.float64) / np.float64(scale)).astype(np.float32)
    cands = [x0]
    up = dn = x0
    for _ in range(2):
        up = np.nextafter(up, np.float32(np.inf)); dn = np.nextafter(dn, np.float32(-np.inf))
        cands += [up, dn]
    c = np.stack(cands)
    return c, (c * np.float32(scale)).astype(np.float32) == y[None]


@pytest.mark.parametrize("sid,sub,N", CASES)
def test_spec_tail(sid, sub, N, monkeypatch):
    import torch

    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.scene import load_bundle

    task = TASKS[sid]
    monkeypatch.setenv("RL_ENV_SUB", sub)

    def make(spec, corrupt=True):
        monkeypatch.setenv("RL_ENV_SPEC", "1" if spec else "0")
        desc, extra = load_bundle(task)
        if not corrupt:
            desc.task.policy_corrupt = 0
        return ManagerBasedRLEnv(desc=desc, extra=extra, num_envs=N, seed=SEED, device="cuda:0")

    a, b, c = make(True), make(False), make(True, corrupt=False)  # the Spec, the interpreter, the Spec's play variant
    assert a._native.spec_id() == sid and c._native.spec_id() == sid and b._native.spec_id() == 0
    assert a._native.envs_per_wavefront() == 16 // int(sub)
    t = a.desc.task
    assert t.policy_corrupt and not c.desc.task.policy_corrupt
    for env in (a, b, c):
        env.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    errs, figures = [], dict(task=task, sub=sub, N=N)

    def step_all(act, shared):
        for env in (b, c):
            env.load_state(shared)
        outs = [env.step(act) for env in (a, b, c)]
        (oa, _, ta, toa, _), (ob, _, tb, tob, _) = outs[0], outs[1]
        assert torch.equal(ta, tb) and torch.equal(toa, tob)
        for grp in ("policy", "critic"):
            x, y = oa[grp].double().cpu().numpy(), ob[grp].double().cpu().numpy()
            errs.append((np.abs(x - y) / np.maximum(np.abs(y), 1.0)).ravel())
        return outs

    # ---- a few steps after reset with small actions: the state of (b) the noise identity and (c) the play variant
    for s in range(4):
        act = 0.1 * (torch.rand(N, a.num_actions, device="cuda", generator=g) * 2 - 1)
        outs = step_all(act, a.read_state())
    noisy, clean = outs[0][0]["policy"].cpu().numpy(), outs[2][0]["policy"].cpu().numpy()
    critic = outs[2][0]["critic"].cpu().numpy()
    sa, sc = a.read_state(), c.read_state()
    for k in ("root_state", "joint_pos", "joint_vel"):  # corruption touches the rows alone: the two Spec envs still share their state
        assert np.asarray(sa[k]).tobytes() == np.asarray(sc[k]).tobytes(), k
    step_count = int(a._native.step_count)
    pol = term_columns(t, "policy", a.num_actions)
    dim = pol[-1][2] + pol[-1][3]
    assert noisy.shape == (N, dim)
    ok_pairs = np.zeros((N, dim), bool)
    worst_ulp = 0.0
    binds = np.zeros((N, dim), bool)
    u = px.uniform(SEED, np.arange(N)[:, None], step_count, px.STREAM_NOISE, np.arange(dim)[None])
    for i, kind, off, w in pol:
        ot = t.policy[i]
        scale, lo, hi = np.float32(ot.scale), np.float32(ot.clip_lo), np.float32(ot.clip_hi)
        n_lo = np.float64(np.float32(ot.noise_lo)) if ot.has_noise else 0.0
        n_rng = np.float64(np.float32(ot.noise_hi) - np.float32(ot.noise_lo)) if ot.has_noise else 0.0
        want = n_lo + n_rng * u[:, off:off + w]
        xn, vn = preimages(noisy[:, off:off + w], scale)
        xc, vc = preimages(clean[:, off:off + w], scale)
        assert vn.any(axis=0).all() and vc.any(axis=0).all(), KIND_NAMES[kind]
        binds[:, off:off + w] = ((xn <= lo) | (xn >= hi)).any(axis=0) | ((xc <= lo) | (xc >= hi)).any(axis=0)
        best = np.full(want.shape, np.inf)
        for p in range(5):
            for q in range(5):
                # the operands of the identity: the two rows' values and the draw (a draw that nearly cancels the value is the largest of them)
                ulp = np.spacing(np.maximum(np.maximum(np.abs(xn[p]), np.abs(xc[q])), np.abs(want).astype(np.float32))).astype(np.float64)
                d = np.abs((xn[p].astype(np.float64) - xc[q].astype(np.float64)) - want) / ulp
                best = np.where(vn[p] & vc[q], np.minimum(best, d), best)
        ok_pairs[:, off:off + w] = best <= 1.0
        worst_ulp = max(worst_ulp, float(np.where(binds[:, off:off + w], 0.0, best).max()))
    figures["noise_cols_clipped"] = float(binds.mean())
    figures["noise_cols_off"], figures["noise_worst_ulp"] = int((~ok_pairs & ~binds).sum()), worst_ulp
    # ---- (c): the play variant's policy row against its critic's columns of the same term
    crit = {kind: (i, off, w) for i, kind, off, w in term_columns(t, "critic", a.num_actions)}
    compared, skipped = [], []
    for i, kind, off, w in pol:
        if kind not in crit:
            skipped.append(KIND_NAMES[kind] + ": not in the critic group")
            continue
        j, coff, cw = crit[kind]
        op, oc = t.policy[i], t.critic[j]
        if (np.float32(op.scale), np.float32(op.clip_lo), np.float32(op.clip_hi)) != (np.float32(oc.scale), np.float32(oc.clip_lo), np.float32(oc.clip_hi)):
            skipped.append(KIND_NAMES[kind] + ": clip / scale differ between the groups")
            continue
        assert cw == w and clean[:, off:off + w].tobytes() == critic[:, coff:coff + w].tobytes(), (task, sub, N, KIND_NAMES[kind])
        compared.append(KIND_NAMES[kind])
    figures["play_terms_bit_equal"], figures["play_terms_skipped"] = compared, skipped
    # ---- (a): env 0 times out
    shared = a.read_state()
    shared["episode_length"] = np.asarray(shared["episode_length"]).copy()
    shared["episode_length"][0] = a.max_episode_length - 1
    a.load_state(shared)
    act = torch.rand(N, a.num_actions, device="cuda", generator=g) * 2 - 1
    outs = step_all(act, shared)
    assert bool(outs[0][3][0]) and bool(outs[1][3][0]), "env 0 did not time out"
    # ---- (a): the push interval due in every env
    shared = a.read_state()
    shared["task_state"] = np.asarray(shared["task_state"]).copy()
    shared["task_state"][:, RL_TS_PUSH_TIME_LEFT] = 0.0
    a.load_state(shared)
    act = torch.rand(N, a.num_actions, device="cuda", generator=g) * 2 - 1
    step_all(act, shared)
    if t.ev_push:  # the push fired: its timer was drawn again
        for env in (a, b):
            assert (np.asarray(env.read_state()["task_state"])[:, RL_TS_PUSH_TIME_LEFT] > 0).all()
    e = np.concatenate(errs)
    figures["obs_max"], figures["obs_p99"], figures["obs_bit_different"] = float(e.max()), float(np.quantile(e, 0.99)), int((e != 0).sum())
    print("\n[spec-tail]", json.dumps(figures))
    for env in (a, b, c):
        env.close()
    assert len(compared) >= 2, figures
    assert figures["noise_cols_clipped"] <= 0.10, figures
    assert figures["noise_cols_off"] == 0, figures
    assert figures["obs_max"] <= OBS_MAX and figures["obs_p99"] <= OBS_P99, figures
