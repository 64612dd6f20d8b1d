"""GPU tier of the HIP recurrent distillation learner (include/rl_distill_bptt.h, robot_lab_amd/distill_recurrent_hip.py) against the torch rule
that defines it (robot_lab_amd/distill_recurrent.py: `RecurrentDistillation.update`, truncated back-propagation through time).

The bound is the project's (tests/distill_helpers.py, tests/bptt_helpers.py): per tensor e = max|got - ref64| / max|ref64| <= 8 d, d = the fp32 torch
rule's own distance from the fp64 torch rule on the CPU.  Bounded: the forward per group, the gradient of every group of the update per parameter
tensor (the four LSTM tensors separately; the device runs the group on the fp64 run's parameters and carried state rounded to fp32, and d is the
fp32 rule on the same), parameters, both Adam moments, the statistic and the final state after a whole update (both loss types, max_grad_norm set
and unset).  Exact: two runs give identical bits, the reset is a select, dones[T - 1] is not read, a group read through the row index equals the
same steps laid out contiguously.  Then the whole loop on the real env, on both learners.  Every case (shape, loss type, clip) has its own
batch seed, chosen on the torch references alone so that the yardstick measures every bounded tensor (distill_recurrent_helpers.yardstick_measures:
d at least half an fp32 spacing, and the fp32 rule by two other fp32 routes within 8 d itself).  `DISTILL_RECURRENT_PARITY_OUT=<file>` appends the
measured multiples (profiles/distill_recurrent_parity.txt)."""
import copy
import os

import numpy as np
import pytest

import distill_recurrent_helpers as dh
from distill_recurrent_helpers import SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLAT = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
NAMES = list(SHAPES)


def _record(lines):
    path = os.environ.get("DISTILL_RECURRENT_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def _hip(name, pol=None, **kw):
    from robot_lab_amd.distill_recurrent_hip import HipRecurrentDistillation

    pol = dh.case(name)[0] if pol is None else pol
    return HipRecurrentDistillation(copy.deepcopy(pol).to(DEV), num_envs=SHAPES[name]["N"], **dh.hyper(name, **kw))


def _batch(name, fields=None, loss_type="mse", max_grad_norm=None):
    import torch

    return dh.as_batch(dh.case(name, loss_type, max_grad_norm)[1] if fields is None else fields, torch.float32, DEV)


def _load(hip, pol, params):
    """the learner's master parameters <- {trained parameter name: fp64 tensor}, rounded to fp32"""
    import torch

    with torch.no_grad():
        for k, p in dh.trained_named(pol):
            p.copy_(params[k].to(device=p.device, dtype=p.dtype))
    hip.load_from(pol)


def _state(st):
    return None if st is None else tuple(t.float().to(DEV) for t in st)


def _np(t):
    return t.detach().double().cpu().numpy()


# ---- bounded ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_parity_per_group(name):
    ref = dh.reference(name)
    hip, batch, lines, bad = _hip(name), _batch(name), [], []
    pol = copy.deepcopy(dh.case(name)[0]).to(DEV)
    print()
    for g, (g64, g32) in enumerate(zip(ref["f64"]["groups"], ref["f32"]["groups"])):
        _load(hip, pol, g64["params"])
        mean, (h, c) = hip.forward(batch, g64["steps"], _state(g64["state_in"]))
        got = dict(mean=_np(mean), h=_np(h), c=_np(c))
        r64 = dict(mean=g64["means"], h=_np(g64["state_out"][0]), c=_np(g64["state_out"][1]))
        r32 = dict(mean=g32["means_at64"], **g32["state_out_at64"])
        bad += dh.within_bound(f"{name} group {g} {g64['steps']}: forward", got, r64, r32, lines)
    hip.close()
    _record(lines)
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_group_grad_parity(name):
    """every group of the update, per parameter tensor, the four LSTM tensors separately; the carried input state is the fp64 rule's"""
    ref = dh.reference(name)
    hip, batch, lines, bad = _hip(name), _batch(name), [], []
    pol = copy.deepcopy(dh.case(name)[0]).to(DEV)
    assert len(ref["f64"]["groups"]) == len(dh.update_groups(SHAPES[name])[0]) >= 1
    print()
    for g, (g64, g32) in enumerate(zip(ref["f64"]["groups"], ref["f32"]["groups"])):
        _load(hip, pol, g64["params"])
        flat, (h, c) = hip.group_grad(batch, g64["steps"], _state(g64["state_in"]))
        got = dh.split_flat(flat, pol)
        assert len([k for k in got if ".rnn." in k]) == 4
        bad += dh.within_bound(f"{name} group {g} {g64['steps']}: group_grad", got, g64["grads"], g32["grads_at64"], lines)
        bad += dh.within_bound(f"{name} group {g} {g64['steps']}: state out", dict(h=_np(h), c=_np(c)), dict(h=_np(g64["state_out"][0]), c=_np(g64["state_out"][1])),
                               g32["state_out_at64"], lines)
    hip.close()
    _record(lines)
    assert not bad, bad


@pytest.mark.parametrize("max_grad_norm", [None, 0.02], ids=["no-clip", "clip"])
@pytest.mark.parametrize("loss_type", ["mse", "huber"])
@pytest.mark.parametrize("name", NAMES)
def test_one_update_parity(name, loss_type, max_grad_norm):
    """parameters, both Adam moments, the behaviour statistic and the final state after one whole update"""
    ref = dh.reference(name, loss_type, max_grad_norm)
    r64, r32 = ref["f64"], ref["f32"]
    if max_grad_norm is not None:  # the clip must bite for the case to mean something (a condition on the reference alone)
        assert max(np.sqrt(sum(float((v ** 2).sum()) for v in g["grads"].values())) for g in r64["groups"]) > max_grad_norm
    hip, batch, pol = _hip(name, loss_type=loss_type, max_grad_norm=max_grad_norm), _batch(name, loss_type=loss_type, max_grad_norm=max_grad_norm), dh.case(name)[0]
    res = hip.update(batch)
    assert set(res) == {"behavior"} and hip.adam_step == hip.num_updates == r64["step"]
    lines, bad = [], []
    title = f"{name} {loss_type} {'clip' if max_grad_norm else 'no-clip'}: one update"
    print()
    for what, flat in (("params", "parameters"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")):
        bad += dh.within_bound(f"{title}, {what}", dh.split_flat(hip.flat(flat), pol), r64[what], r32[what], lines)
    bad += dh.within_bound(f"{title}, final state", dict(h=_np(hip.final_state[0]), c=_np(hip.final_state[1])), r64["final_state"], r32["final_state"], lines)
    # the statistic is ONE scalar, and the seed rule (distill_recurrent_helpers.case_seed) does not look at it: where the fp32 rule's value happens to
    # round closer than the yardstick's own floor, d is the floor (half an fp32 spacing, below which d measures nothing)
    b64, b32 = r64["result"]["behavior"], r32["result"]["behavior"]
    b32 = b32 if abs(b32 - b64) >= dh.YARDSTICK_FLOOR * abs(b64) else b64 * (1.0 + dh.YARDSTICK_FLOOR)
    bad += dh.within_bound(f"{title}, statistic", dict(behavior=np.array([res["behavior"]])), dict(behavior=np.array([b64])), dict(behavior=np.array([b32])), lines)
    hip.close()
    _record(lines)
    assert not bad, bad


# ---- exact -----------------------------------------------------------------------------------------------------------------------------------
def _everything(hip):
    return [hip.flat(w).clone() for w in ("parameters", "exp_avg", "exp_avg_sq")] + [t.clone() for t in hip.final_state]


@pytest.mark.parametrize("name", ["ragged", "real-widths"])
def test_two_updates_from_the_same_state_are_bit_identical(name):
    import torch

    runs = []
    for _ in range(2):
        hip = _hip(name, max_grad_norm=0.02)
        res = hip.update(_batch(name))
        runs.append((res["behavior"], _everything(hip)))
        hip.close()
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def _edited(name, **changes):
    f = {k: np.array(v) for k, v in dh.case(name)[1].items()}
    for k, fn in changes.items():
        fn(f[k])
    return f


@pytest.mark.parametrize("name", ["ragged", "4H-crosses-128"])
def test_the_reset_is_a_select(name):
    """NaN in the old state of a row behind a done reaches no output: planted in the carried state of a group whose first step follows a done"""
    import torch

    dones = dh.case(name)[1]["dones"]
    ref = dh.reference(name)["f64"]["groups"]
    hip, batch = _hip(name), _batch(name)
    checked = 0
    for g64 in ref:
        t0 = g64["steps"][0]
        if t0 == 0 or not dones[t0 - 1].any():
            continue
        gone = torch.as_tensor(dones[t0 - 1]).to(DEV)
        h, c = _state(g64["state_in"])
        clean = hip.group_grad(batch, g64["steps"], (h, c))
        hn, cn = h.clone(), c.clone()
        hn[gone], cn[gone] = float("nan"), float("nan")
        dirty = hip.group_grad(batch, g64["steps"], (hn, cn))
        mean_c, _ = hip.forward(batch, g64["steps"], (h, c))
        mean_d, _ = hip.forward(batch, g64["steps"], (hn, cn))
        assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1][0], dirty[1][0]) and torch.equal(clean[1][1], dirty[1][1]) and torch.equal(mean_c, mean_d)
        assert bool(torch.isfinite(dirty[0]).all())
        checked += 1
    assert checked >= 1, "no group of the case starts behind a done"
    hip.close()


def test_the_last_dones_are_not_read():
    import torch

    name = "ragged"
    outs = []
    for flip in (False, True):
        f = _edited(name, dones=(lambda d: d.__setitem__(-1, ~d[-1])) if flip else (lambda d: None))
        hip = _hip(name)
        res = hip.update(_batch(name, f))
        outs.append((res["behavior"], _everything(hip)))
        hip.close()
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_a_wrapping_group_equals_the_same_steps_laid_out_contiguously():
    """Steps (3, 4, 0, 1) of a storage, read through the row index, against steps (0, 1, 2, 3) of a second storage that holds the same rows in that
    order, one contiguous row range.  The first storage's (h0, c0) is zero and every row of its step 4 is done, so the second storage's step 2
    starts from zeros behind a done of every row exactly as the first's epoch starts from (h0, c0), and no gradient crosses either: gradient,
    means and output state agree bit for bit."""
    import torch

    name = "ragged"
    s = SHAPES[name]
    f = {k: np.array(v) for k, v in dh.case(name)[1].items()}
    f["dones"][4] = True
    f["h0"][:], f["c0"][:] = 0.0, 0.0
    order = [3, 4, 0, 1, 2]
    g = {k: (np.ascontiguousarray(v[order]) if k in ("observations", "teacher_actions", "dones") else v) for k, v in f.items()}
    state = tuple(0.3 * torch.randn(s["N"], s["H"], generator=torch.Generator().manual_seed(5)).to(DEV) for _ in range(2))
    gone = torch.as_tensor(f["dones"][2]).to(DEV).unsqueeze(-1)  # the reset of the first storage's step 3, applied by hand for the second's step 0
    pre = tuple(torch.where(gone, torch.zeros_like(t), t) for t in state)
    g["h0"], g["c0"] = pre[0].cpu().numpy(), pre[1].cpu().numpy()
    hip = _hip(name, gradient_length=4)
    fa, fb = _batch(name, f), _batch(name, g)
    grad_a, st_a = hip.group_grad(fa, [3, 4, 0, 1], state)
    mean_a, _ = hip.forward(fa, [3, 4, 0, 1], state)
    grad_b, st_b = hip.group_grad(fb, [0, 1, 2, 3], None)
    mean_b, _ = hip.forward(fb, [0, 1, 2, 3], None)
    assert bool(grad_a.abs().sum() > 0)
    assert torch.equal(grad_a, grad_b) and torch.equal(mean_a, mean_b) and torch.equal(st_a[0], st_b[0]) and torch.equal(st_a[1], st_b[1])
    hip.close()


def test_optimizer_state_crosses_the_learners():
    """the HIP learner's optimiser state loads into torch.optim.Adam(trained_parameters()) and back"""
    import torch

    from robot_lab_amd.distill_recurrent import RecurrentDistillation

    name = "ragged"
    hip, batch = _hip(name), _batch(name)
    hip.update(batch)
    d = hip.optimizer_state_dict()
    pol = hip.store_into(copy.deepcopy(dh.case(name)[0]).to(DEV))
    alg = RecurrentDistillation(pol, **dh.hyper(name))
    alg.optimizer.load_state_dict(d)
    assert len(alg.optimizer.state) == len(pol.trained_parameters())
    other = _hip(name)
    other.load_from(pol)
    other.load_optimizer_state_dict(alg.optimizer.state_dict())
    a, b = hip.update(batch), other.update(batch)
    assert a == b and all(torch.equal(x, y) for x, y in zip(_everything(hip), _everything(other)))
    hip.close(); other.close()


# ---- the real env: A1 Flat, 64 envs x 8 steps ------------------------------------------------------------------------------------------------
N_ENV, T_ENV = 64, 8
MODEL = dict(class_name="RNNModel", hidden_dims=[128, 128, 128], activation="elu", obs_normalization=False, rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)
CFG = dict(class_name="DistillationRunner", seed=3, num_steps_per_env=T_ENV, save_interval=100, obs_groups={"student": ["policy"], "teacher": ["policy"]},
           student=dict(MODEL, distribution_cfg=dict(class_name="GaussianDistribution", init_std=0.1)),
           teacher=dict(MODEL, distribution_cfg=dict(class_name="GaussianDistribution", init_std=0.0)),
           algorithm=dict(class_name="Distillation", num_learning_epochs=2, learning_rate=1e-3, gradient_length=15, optimizer="adam", loss_type="mse"))


def _env(seed=3):
    from robot_lab_amd.env import ManagerBasedRLEnv

    return ManagerBasedRLEnv(FLAT, num_envs=N_ENV, seed=seed, device=DEV)


def _arm(env):
    """time-outs over the first 24 steps (after the constructor's reset): dones inside every window of three iterations and at their last steps"""
    import torch

    env.episode_length_buf = env.max_episode_length - 1 - (torch.arange(N_ENV) % 24)
    return env


@pytest.fixture(scope="module")
def recurrent_teacher(tmp_path_factory):
    """a recurrent teacher: two PPO iterations of `Trainer(rnn_type="lstm")`, saved in the runner's checkpoint layout"""
    import torch

    from robot_lab_amd.ppo import Trainer

    env = _env(seed=42)
    tr = Trainer(env, seed=42, num_steps_per_env=T_ENV, rnn_type="lstm", rnn_hidden_dim=256, actor_hidden=(128, 128, 128), critic_hidden=(128, 128, 128),
                 num_learning_epochs=2)
    _arm(env)
    for _ in range(2):
        tr.iterate()
    sd = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
    path = str(tmp_path_factory.mktemp("recurrent_teacher") / "model_2.pt")
    torch.save({"model_state_dict": sd, "optimizer_state_dict": None, "iter": 2, "infos": None}, path)
    tr.recurrent.close(); tr.storage.close(); env.close()
    return path, sd


def _runner(monkeypatch, learner, cfg=None):
    import types

    from robot_lab_amd import shims

    shims.install()
    from rsl_rl.runners import DistillationRunner

    monkeypatch.setenv("RL_LEARNER", learner)
    runner = DistillationRunner(types.SimpleNamespace(unwrapped=_env()), CFG if cfg is None else cfg, log_dir=None, device=DEV)
    _arm(runner.trainer.env)
    return runner


def _optimizer_state(runner):
    from robot_lab_amd.ppo_hip import adam_state_flat

    alg = runner.alg
    d = alg.optimizer_state_dict() if hasattr(alg, "optimizer_state_dict") else alg.optimizer.state_dict()
    m1, m2, step, lr = adam_state_flat(d, [tuple(p.shape) for p in alg.policy.trained_parameters()])
    return m1.cpu(), m2.cpu(), step, lr


@pytest.mark.parametrize("learner", ["torch", "hip"])
def test_runner_distils_a_recurrent_teacher_on_the_real_env(learner, monkeypatch, recurrent_teacher):
    import torch

    import recurrent_helpers as rh

    path, sd = recurrent_teacher
    runner = _runner(monkeypatch, learner)
    tr, pol = runner.trainer, runner.alg.policy
    assert type(runner.alg).__name__ == ("HipRecurrentDistillation" if learner == "hip" else "RecurrentDistillation") and tr.recurrent and tr.teacher_recurrent
    with pytest.raises(ValueError, match="load"):
        runner.learn(1)
    runner.load(path)
    assert runner.current_learning_iteration == 0  # a teacher's checkpoint is not a resume
    for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        assert torch.equal(pol.memory_t.rnn.state_dict()[k].cpu(), sd[f"memory_a.rnn.{k}"]), k
    assert torch.equal(pol.teacher[0].weight.detach().cpu(), sd["actor.0.weight"])
    runner.learn(2)
    assert all(np.isfinite(h[k]) for h in runner.history for k in ("behavior", "mean_reward", "done_rate", "learning_rate", "grad_norm"))
    # the hand-off: the collector's student state is the learner's final state, bit for bit
    col = tr.collector
    for a, b in zip(col.student_state(), runner.alg.final_state):
        assert torch.equal(a, b)
    assert runner.alg.num_updates == (1 if learner == "hip" else 2)  # one optimiser step per update (16 steps, gradient length 15); the torch rule counts on
    # a third collection, replayed in fp64 from the stored observations and dones
    teacher_state = (col._ht[col._k].clone(), col._ct[col._k].clone())
    first_reset = col.reset.clone().bool()
    assert bool(first_reset.any()), "no done at the last step of the previous iteration"
    col.collect()
    torch.cuda.synchronize()
    st = tr.storage
    assert bool(st.dones[:-1].any())
    assert bool((col.h0[first_reset] == 0).all()) and bool((col.c0[first_reset] == 0).all())          # exactly zero behind a done
    assert bool((col.h0[~first_reset] != 0).any(-1).all())
    d = st.dones.cpu().bool()
    reset = torch.cat([torch.zeros_like(d[:1]), d[:-1]], 0)
    keep = (~first_reset).float().unsqueeze(-1)
    bad = []
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        m = copy.deepcopy(pol).cpu().to(dt)
        with torch.no_grad():
            hs, _ = m.memory_s(st.observations.cpu().to(dt), col.h0.cpu().to(dt), col.c0.cpu().to(dt), reset)
            ht, _ = m.memory_t(st.privileged_observations.cpu().to(dt), (teacher_state[0] * keep).cpu().to(dt), (teacher_state[1] * keep).cpu().to(dt), reset)
            out = (m.student(hs), m.teacher(ht))
        if name == "64":
            ref = out
    for k, got, i in (("student mean", st.mu, 0), ("teacher actions", col.teacher_actions, 1)):
        ok, line = rh.bound_check(k, got.cpu().numpy(), ref[i].numpy(), out[i].numpy())
        if not ok:
            bad.append(line)
    assert not bad, "\n".join([rh.BOUND_HEADER] + bad)
    # the inference policy is stateful and resets rows
    policy = runner.get_inference_policy()
    obs = tr.env.get_observations()
    with torch.inference_mode():  # (as play.py calls it)
        y0 = policy(obs).clone()
        y1 = policy(obs).clone()
        policy.reset(torch.ones(N_ENV, dtype=torch.bool, device=DEV))
        y2 = policy(obs).clone()
    assert not torch.equal(y0, y1) and torch.equal(y0, y2) and hasattr(policy, "reset")
    tr.env.close()


def test_real_env_checkpoints_cross_the_two_learners(monkeypatch, tmp_path, recurrent_teacher):
    import torch

    a, b = _runner(monkeypatch, "hip"), _runner(monkeypatch, "torch")
    for r in (a, b):
        r.load(recurrent_teacher[0])
    for src, dst, its in ((a, b, 2), (b, a, 1)):
        src.learn(num_learning_iterations=its)
        path = str(tmp_path / f"model_{src.current_learning_iteration}_{its}.pt")
        src.save(path)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert ck["optimizer_state_dict"]["state"] and ck["iter"] == src.current_learning_iteration
        assert {k.split(".")[0] for k in ck["model_state_dict"]} == {"memory_s", "student", "memory_t", "teacher", "std"}
        dst.load(path)
        assert dst.current_learning_iteration == src.current_learning_iteration
        if hasattr(dst.alg, "store_into"):
            dst.alg.store_into(dst.alg.policy)  # (what the learner holds, not what load_state_dict put into the module)
        for (k, p), q in zip(src.alg.policy.state_dict().items(), dst.alg.policy.state_dict().values()):
            assert torch.equal(p, q), k
        s, d = _optimizer_state(src), _optimizer_state(dst)
        assert torch.equal(s[0], d[0]) and torch.equal(s[1], d[1]) and s[2:] == d[2:] and s[2] > 0, (s[2:], d[2:])
    a.trainer.env.close(); b.trainer.env.close()


def _trainer(use_graph, teacher_sd, **kw):
    from robot_lab_amd.distill import DistillTrainer

    tr = DistillTrainer(_env(), **{**dict(num_steps_per_env=T_ENV, student_hidden=(128, 128, 128), teacher_hidden=(128, 128, 128), init_noise_std=0.1, seed=3,
                                          use_graph=use_graph, num_learning_epochs=2, gradient_length=15, learning_rate=1e-3, rnn_type="lstm", rnn_hidden_dim=256), **kw})
    tr.load_state_dict(teacher_sd)
    _arm(tr.env)
    return tr


def test_real_env_captured_replay_equals_the_eager_loop_bit_for_bit(recurrent_teacher):
    import torch

    eager, graph = _trainer(False, recurrent_teacher[1]), _trainer(True, recurrent_teacher[1])
    for _ in range(3):  # the captured side: eager warm-up, capture + replay, replay
        eager.collector.collect()
        graph.collector.collect()
    assert graph.collector._graph is not None and eager.collector._graph is None
    torch.cuda.synchronize()
    snap = lambda t: {k: getattr(t.storage, k).clone() for k in ("observations", "privileged_observations", "actions", "mu", "rewards", "dones")} | dict(  # noqa: E731
        teacher_actions=t.collector.teacher_actions.clone(), h0=t.collector.h0.clone(), c0=t.collector.c0.clone(), reset=t.collector.reset.clone(),
        h=t.collector.student_state()[0].clone(), c=t.collector.student_state()[1].clone())
    a, b = snap(eager), snap(graph)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert float(a["teacher_actions"].abs().max()) > 0 and bool(a["dones"].any())
    eager.env.close(); graph.env.close()


@pytest.mark.parametrize("learner", ["torch", "hip"])
def test_real_env_a_feed_forward_teacher_runs_the_same_loop(learner):
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(11)
    ac = ActorCritic(45, 45, 12, actor_hidden=(128, 64), critic_hidden=(32,))
    tr = _trainer(True, ac.state_dict(), teacher_recurrent=False, teacher_hidden=(128, 64), learner=learner)
    assert tr.cell_t is None and not tr.policy.teacher_recurrent
    rows = [tr.iterate() for _ in range(3)]
    assert all(np.isfinite(r[k]) for r in rows for k in ("behavior", "grad_norm", "mean_reward"))
    for a, b in zip(tr.collector.student_state(), tr.alg.final_state):
        assert torch.equal(a, b)
    # the stored teacher actions are the feed-forward teacher's on the stored rows (the inference bound of tests/test_gpu_recurrent.py)
    import recurrent_helpers as rh

    rows = tr.storage.privileged_observations.cpu()
    with torch.no_grad():
        t64, t32 = copy.deepcopy(tr.policy.teacher).cpu().double()(rows.double()), copy.deepcopy(tr.policy.teacher).cpu()(rows)
    ok, line = rh.bound_check("feed-forward teacher actions", tr.collector.teacher_actions.cpu().numpy(), t64.numpy(), t32.numpy())
    assert ok, "\n".join([rh.BOUND_HEADER, line])
    off = _trainer(True, ac.state_dict(), teacher_recurrent=False, teacher_hidden=(128, 64), learner=learner, carry_learner_state=False)
    off.iterate()
    assert not torch.equal(off.collector.student_state()[0], off.alg.final_state[0])  # the collection keeps its own cells' state
    tr.env.close(); off.env.close()
