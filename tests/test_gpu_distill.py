"""GPU tier of distillation: the HIP learner (include/rl_distill.h) exactly on the integer family and within the project's bound of the unchanged
torch rule in fp64, the collection loop (captured replay = eager loop, the teacher's actions), and the runner end to end with each learner.

The bound (tests/distill_helpers.py `within_bound`): per tensor e <= 8 d, e the HIP learner's and d the fp32 torch rule's own distance from the
fp64 torch rule, both relative to max|ref64|.  With DISTILL_PARITY_OUT=<file> in the
environment the measured multiples are written there (profiles/distill_parity.txt)."""
import copy
import os
import types

import numpy as np
import pytest

from distill_helpers import EX, SHAPES, cast_case, exact_group_gradient, exact_policy, float_case, recorded_update, split_student, within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A1F = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
LINES = []


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    out = os.environ.get("DISTILL_PARITY_OUT")
    if out and LINES:
        with open(out, "w") as f:
            f.write("HIP distillation learner against the torch rule (robot_lab_amd/distill.py) in fp64; d: the fp32 torch rule's own distance\n"
                    f"{'case':<44}{'tensor':<12}{'max|ref64|':>12}{'e (hip)':>12}{'d (torch32)':>12}{'e/d':>8}{'floor':>12}\n" + "\n".join(LINES) + "\n")


def _hip(pol, batch, **kw):
    from robot_lab_amd.distill_hip import HipDistillation

    p = copy.deepcopy(pol).to(DEV)
    b = types.SimpleNamespace(observations=batch.observations.to(DEV).contiguous(), teacher_actions=batch.teacher_actions.to(DEV).contiguous())
    return HipDistillation(p, num_envs=b.observations.shape[1], **kw), b


def _state(alg):
    import torch

    torch.cuda.synchronize()
    return {k: alg.flat(k).cpu() for k in ("parameters", "exp_avg", "exp_avg_sq")}


# ---- exact, no tolerance
def test_group_gradient_is_the_int64_result_bit_for_bit():
    pol, batch = exact_policy()
    alg, b = _hip(pol, batch, num_learning_epochs=EX["epochs"], gradient_length=EX["gradient_length"])
    for steps in [(0, 1, 2), (3, 4, 0)]:  # one contiguous row range; the wrap through the row index
        got = alg.group_grad(b, steps).cpu().numpy()
        assert np.array_equal(got.view(np.int32), exact_group_gradient(steps).view(np.int32)), steps
    alg.close()


def test_two_updates_from_the_same_state_agree_bit_for_bit_and_no_clip_is_a_coefficient_of_one():
    import torch

    pol, batch = exact_policy()
    kw = dict(num_learning_epochs=EX["epochs"], gradient_length=EX["gradient_length"], learning_rate=1e-3)
    runs = []
    for extra in ({}, {}, dict(max_grad_norm=1e30)):
        alg, b = _hip(pol, batch, **kw, **extra)
        res = alg.update(b)
        assert alg.num_updates == 3 and alg.adam_step == 3
        runs.append((res, alg.last_grad_norm, _state(alg)))
        alg.close()
    for res, norm, st in runs[1:]:
        assert res == runs[0][0] and norm == runs[0][1] and norm > 0
        for k, v in st.items():
            assert torch.equal(v.view(torch.int32), runs[0][2][k].view(torch.int32)), k
    assert not torch.equal(runs[0][2]["parameters"], torch.cat([p.detach().reshape(-1) for p in pol.student.parameters()]))


# ---- bounded against the unchanged torch rule in fp64
def _references(pol, batch, s, step, **kw):
    """{dtype: (result, per-step gradients, learner)} of the torch rule on the host"""
    import torch

    from robot_lab_amd.distill import Distillation

    out = {}
    for dtype in (torch.float64, torch.float32):
        p, b = cast_case(pol, batch, dtype, "cpu")
        alg = Distillation(p, num_learning_epochs=s["epochs"], gradient_length=s["gradient_length"], learning_rate=1e-3, **kw)
        res, grads, _ = recorded_update(alg, b, step=step)
        out[dtype] = (res, grads, alg)
    return out


def _adam(alg):
    """{student parameter name: (exp_avg, exp_avg_sq)} of a torch learner's optimiser"""
    return {n: (alg.optimizer.state[p]["exp_avg"].detach().double().cpu(), alg.optimizer.state[p]["exp_avg_sq"].detach().double().cpu())
            for n, p in alg.policy.student.named_parameters()}


@pytest.mark.parametrize("variant", ["mse", "huber", "clip"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_hip_learner_is_within_the_bound_of_the_fp64_rule(name, variant):
    import torch

    from robot_lab_amd.distill import update_groups

    s = SHAPES[name]
    pol, batch = float_case(name, huber=variant == "huber")
    kw = dict(loss_type="huber") if variant == "huber" else {}
    title = f"{name} {variant}"
    bad = []
    # the gradient of every group, at the case's parameters
    ref = _references(pol, batch, s, False, **kw)
    groups, left = update_groups(s["T"], s["gradient_length"], s["epochs"])
    assert len(ref[torch.float64][1]) == len(groups) and (name != "ragged" or (left and any(g[0] > g[-1] for g in groups)))
    alg, b = _hip(pol, batch, num_learning_epochs=s["epochs"], gradient_length=s["gradient_length"], learning_rate=1e-3, **kw)
    for i, steps in enumerate(groups):
        got = split_student(alg.group_grad(b, steps), pol)
        r64, r32 = (split_student(ref[d][1][i], pol) for d in (torch.float64, torch.float32))
        bad += within_bound(f"{title} grad {steps}", got, r64, r32, LINES)
    if variant == "clip":  # small enough that the clip coefficient is below 0.5 in every step (asserted on the fp64 rule's own norms)
        kw["max_grad_norm"] = 0.25 * min(float(g.norm()) for g in ref[torch.float64][1])
    # one whole update: parameters, both Adam moments, behavior
    ref = _references(pol, batch, s, True, **kw)
    if variant == "clip":
        assert all(kw["max_grad_norm"] / n < 0.5 for n in ref[torch.float64][2].grad_norms) and len(ref[torch.float64][2].grad_norms) == len(groups)
    alg.close()
    alg, b = _hip(pol, batch, num_learning_epochs=s["epochs"], gradient_length=s["gradient_length"], learning_rate=1e-3, **kw)
    res = alg.update(b)
    assert alg.num_updates == len(groups)
    st = _state(alg)
    r64, r32 = ref[torch.float64][2], ref[torch.float32][2]
    params = lambda a: {n: p.detach().double().cpu() for n, p in a.policy.student.named_parameters()}  # noqa: E731
    bad += within_bound(f"{title} parameters", split_student(st["parameters"], pol), params(r64), params(r32), LINES)
    for j, key in enumerate(("exp_avg", "exp_avg_sq")):
        bad += within_bound(f"{title} {key}", split_student(st[key], pol), {n: v[j] for n, v in _adam(r64).items()}, {n: v[j] for n, v in _adam(r32).items()}, LINES)
    bad += within_bound(f"{title} behavior", dict(behavior=res["behavior"]), dict(behavior=ref[torch.float64][0]["behavior"]),
                        dict(behavior=ref[torch.float32][0]["behavior"]), LINES)
    bad += within_bound(f"{title} grad norm", dict(norm=alg.last_grad_norm), dict(norm=r64.last_grad_norm), dict(norm=r32.last_grad_norm), LINES)
    alg.close()
    assert not bad, bad


# ---- collection
def _collector(use_graph, normalizer_state=None, T=4, N=64, seed=5):
    import torch

    from robot_lab_amd.distill_collect import DistillCollector
    from robot_lab_amd.env import ManagerBasedRLEnv
    from robot_lab_amd.policy import MlpPolicy
    from robot_lab_amd.rollout import RolloutStorage

    env = ManagerBasedRLEnv(A1F, num_envs=N, seed=seed, device=DEV)
    obs, _ = env.reset()
    od, A = obs["policy"].shape[1], env.num_actions
    rng = np.random.default_rng(0)
    nets = []
    for dims in ([od, 64, 32, A], [od, 128, 64, A]):
        ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
        bs = [(0.1 * rng.standard_normal(d)).astype(np.float32) for d in dims[1:]]
        nets.append(MlpPolicy(ws, bs, "elu", device=DEV))
    norm = None
    if normalizer_state is not None:
        from robot_lab_amd.obsnorm import ObsNormalizer

        norm = ObsNormalizer(od, 1e-2, max_rows=N, device=DEV)
        norm.set_state(*normalizer_state)
    st = RolloutStorage(N, T, od, od, A, seed=seed, device=DEV)
    std = torch.full((A,), 0.1, device=DEV)
    col = DistillCollector(env, nets[0], nets[1], st, std, normalizer=norm, use_graph=use_graph, clip_actions=100.0)
    return types.SimpleNamespace(env=env, student=nets[0], teacher=nets[1], storage=st, collector=col, normalizer=norm)


def _snapshot(c):
    st = c.storage
    return {k: getattr(st, k).clone() for k in ("observations", "privileged_observations", "actions", "rewards", "dones")} | dict(teacher_actions=c.collector.teacher_actions.clone())


def test_a_captured_replay_equals_the_eager_loop_bit_for_bit():
    import torch

    eager, graph = _collector(False), _collector(True)
    for _ in range(3):  # the captured side: eager warm-up, capture + replay, replay
        eager.collector.collect()
        graph.collector.collect()
    assert graph.collector._graph is not None and eager.collector._graph is None
    torch.cuda.synchronize()
    a, b = _snapshot(eager), _snapshot(graph)
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert float(a["teacher_actions"].abs().max()) > 0 and float(graph.storage.values.abs().max()) == 0.0
    # the stored teacher actions are the teacher's on the stored teacher rows
    for t in range(4):
        want = graph.teacher(graph.storage.privileged_observations[t].contiguous()).clone()
        assert torch.equal(want.view(torch.int32), b["teacher_actions"][t].view(torch.int32)), t


def test_the_teachers_normaliser_is_applied_and_never_updated():
    import torch

    g = torch.Generator().manual_seed(2)
    mean, var = 0.3 * torch.randn(45, generator=g), 0.5 + torch.rand(45, generator=g)
    c = _collector(True, normalizer_state=(mean, var, var.sqrt(), 1234))
    for _ in range(2):
        c.collector.collect()
    torch.cuda.synchronize()
    rows = c.storage.privileged_observations
    assert torch.equal(rows.view(torch.int32), c.storage.observations.view(torch.int32))  # RAW rows in the teacher's slot (both read "policy")
    for t in range(4):
        want = c.teacher(c.normalizer.apply(rows[t].contiguous())).clone()
        assert torch.equal(want.view(torch.int32), c.collector.teacher_actions[t].view(torch.int32)), t
    m, v, s, n = c.normalizer.get_state()
    assert n == 1234 and torch.equal(m.cpu().reshape(-1), mean) and torch.equal(v.cpu().reshape(-1), var) and torch.equal(s.cpu().reshape(-1), var.sqrt())


# ---- end to end
T_E2E, N_E2E = 8, 256
STATE_KEYS = {"std"} | {f"{net}.{2 * l}.{w}" for net, depth in (("student", 3), ("teacher", 3)) for l in range(depth) for w in ("weight", "bias")}


def _cfg():
    model = lambda hidden, std: dict(class_name="MLPModel", hidden_dims=hidden, activation="elu", obs_normalization=False,  # noqa: E731
                                     distribution_cfg=dict(class_name="GaussianDistribution", init_std=std))
    return dict(class_name="DistillationRunner", seed=3, num_steps_per_env=T_E2E, save_interval=100, obs_groups={"student": ["policy"], "teacher": ["policy"]},
                student=model([64, 64], 0.1), teacher=model([128, 64], 0.0),
                algorithm=dict(class_name="Distillation", num_learning_epochs=2, learning_rate=1e-3, gradient_length=4, optimizer="adam"))


def _runner(monkeypatch, learner, log_dir=None):
    from robot_lab_amd import shims
    from robot_lab_amd.env import ManagerBasedRLEnv

    shims.install()
    from rsl_rl.runners import DistillationRunner

    monkeypatch.setenv("RL_LEARNER", learner)
    env = types.SimpleNamespace(unwrapped=ManagerBasedRLEnv(A1F, num_envs=N_E2E, seed=3, device=DEV))
    return DistillationRunner(env, _cfg(), log_dir=log_dir, device=DEV)


@pytest.fixture(scope="module")
def teacher_checkpoint(tmp_path_factory):
    """a randomly initialised ActorCritic in the PPO runner's checkpoint layout"""
    import torch

    from robot_lab_amd.ppo import ActorCritic

    torch.manual_seed(11)
    ac = ActorCritic(45, 45 + 3, 12, actor_hidden=(128, 64), critic_hidden=(32,))
    path = str(tmp_path_factory.mktemp("teacher") / "model_7.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": torch.optim.Adam(ac.parameters()).state_dict(), "iter": 7, "infos": None}, path)
    return path, ac


@pytest.mark.parametrize("learner", ["torch", "hip"])
def test_runner_distils_a_teacher_end_to_end(learner, monkeypatch, tmp_path, teacher_checkpoint):
    import torch

    path, ac = teacher_checkpoint
    runner = _runner(monkeypatch, learner, log_dir=str(tmp_path))
    from isaaclab_rl.rsl_rl import export_policy_as_jit

    assert type(runner.alg).__name__ == ("HipDistillation" if learner == "hip" else "Distillation")
    with pytest.raises(ValueError, match="load"):
        runner.learn(1)
    runner.add_git_repo_to_log(__file__)
    runner.load(path)
    assert runner.current_learning_iteration == 0  # a teacher's checkpoint is not a resume
    runner.learn(10)
    assert runner.history[-1]["behavior"] < runner.history[0]["behavior"], [h["behavior"] for h in runner.history]
    assert all(np.isfinite(h[k]) for h in runner.history for k in ("behavior", "mean_reward", "done_rate", "learning_rate", "grad_norm"))
    pol = runner.alg.policy
    for k, v in ac.actor.state_dict().items():
        assert torch.equal(pol.teacher.state_dict()[k].cpu(), v), k
    assert torch.equal(pol.std.detach().cpu(), torch.full((12,), 0.1))
    d = torch.load(os.path.join(str(tmp_path), "model_10.pt"), map_location="cpu", weights_only=False)
    assert set(d["model_state_dict"]) == STATE_KEYS and d["iter"] == 10
    steps = {int(float(e["step"])) for e in d["optimizer_state_dict"]["state"].values()}
    assert steps == {10 * (2 * T_E2E // 4)} and len(d["optimizer_state_dict"]["state"]) == 6
    obs = runner.env.unwrapped.get_observations()["policy"].clone()
    mean = pol.student(obs).detach()
    y = runner.get_inference_policy()(obs).clone()
    torch.testing.assert_close(y, mean, rtol=2e-5, atol=2e-5)  # the inference kernel's bound of the torch forward (tests/test_gpu_train.py)
    assert torch.equal(runner.get_inference_policy()({"policy": obs}), y)
    export_policy_as_jit(pol, path=str(tmp_path), filename="student.pt")
    jit = torch.jit.load(os.path.join(str(tmp_path), "student.pt"))
    torch.testing.assert_close(jit(obs.cpu()), mean.cpu(), rtol=0, atol=1e-5)
    # the other learner resumes this checkpoint, the optimiser's step count carried
    other = _runner(monkeypatch, "torch" if learner == "hip" else "hip")
    other.load(os.path.join(str(tmp_path), "model_10.pt"))
    assert other.current_learning_iteration == 10
    other.learn(1)
    od = other.alg.optimizer_state_dict() if learner == "torch" else other.alg.optimizer.state_dict()
    assert {int(float(e["step"])) for e in od["state"].values()} == {11 * (2 * T_E2E // 4)}
    assert np.isfinite(other.history[-1]["behavior"])


def test_a_resumed_hip_runner_continues_bit_for_bit(monkeypatch, tmp_path, teacher_checkpoint):
    """A second runner that loads the first one's checkpoint holds the same learner: given the batch the first runner collects next, both take
    the same update bit for bit - parameters, both Adam moments, statistics, the student's inference image.  (The comparison is on the batch of
    ONE env: a checkpoint carries the learner, not the simulator's state.)"""
    import torch

    path, _ = teacher_checkpoint
    one = _runner(monkeypatch, "hip", log_dir=str(tmp_path))
    one.load(path)
    one.learn(2)
    two = _runner(monkeypatch, "hip")
    two.load(os.path.join(str(tmp_path), "model_2.pt"))
    assert two.current_learning_iteration == 2
    for k in ("parameters", "exp_avg", "exp_avg_sq"):
        assert torch.equal(one.alg.flat(k).view(torch.int32), two.alg.flat(k).view(torch.int32)), k
    one.trainer.collector.collect()
    batch = one.trainer.batch
    ra, rb = one.alg.update(batch), two.alg.update(batch)
    assert ra == rb and one.alg.last_grad_norm == two.alg.last_grad_norm and one.alg.adam_step == two.alg.adam_step == 3 * (2 * T_E2E // 4)
    for k in ("parameters", "exp_avg", "exp_avg_sq"):
        assert torch.equal(one.alg.flat(k).view(torch.int32), two.alg.flat(k).view(torch.int32)), k
    one.trainer._push()
    two.trainer._push()
    obs = batch.observations[0].contiguous()
    assert torch.equal(one.trainer.student(obs).view(torch.int32), two.trainer.student(obs).view(torch.int32))
