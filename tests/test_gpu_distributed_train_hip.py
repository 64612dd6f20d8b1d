"""`-m gpu`: tests/test_gpu_distributed_train.py::test_two_ranks_train_one_model with `RL_LEARNER=hip` - two ranks of the reference's
`train.py --distributed` body on the HIP learner (`HipPPO(group=LearnerGroup)`: rl_ppo_minibatch_local -> ONE all-reduce of the wire ->
rl_ppo_minibatch_apply per mini-batch), the checkpoint rank 0 writes, and a second launch that resumes from it through the runner's `load()`.
A box with one GPU holds both ranks under `RL_SHARE_GPU=1` (collectives over gloo); with two or more the same test runs RCCL unchanged."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(script, nproc, out_dir, args, share, records, **extra):
    env = dict(os.environ, RL_TEST_OUT=str(out_dir), HSA_ENABLE_IPC_MODE_LEGACY="0", RL_LEARNER="hip", **extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "RL_SHARE_GPU"):
        env.pop(k, None)
    if share:
        env["RL_SHARE_GPU"] = "1"
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc_per_node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", script), *args]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return [json.load(open(os.path.join(str(out_dir), records.format(r)))) for r in range(nproc)], p


def test_two_ranks_train_one_model_on_the_hip_learner_and_resume(tmp_path):
    import torch

    share = torch.cuda.device_count() < 2
    recs, p = _launch("train_body_rank.py", 2, tmp_path, ["--distributed", "--num_envs", "64", "--max_iterations", "2", "--headless"], share, "rank{}.json")
    for r, rec in enumerate(recs):
        assert rec["world"] == 2 and rec["launcher_local_rank"] == r and rec["agent_device"] == f"cuda:{r}" and rec["env_seed"] == 42 + r
        assert rec["backend"] == ("gloo" if share else "nccl") and rec["iterations"] == 2 and rec["finite"]
    a, b = recs
    assert a["param_sha"] == b["param_sha"], "the two learners drifted apart: the all-reduce of the wire is not tying them together"
    assert a["learning_rate"] == b["learning_rate"]
    assert a["reward_sha"] != b["reward_sha"]  # ... while every rank simulated its own environments (seed 42 + rank)
    # rank 0 alone logs and checkpoints
    path = os.path.join(str(tmp_path), "logs", "model_2.pt")
    assert os.path.isfile(path) and p.stdout.count("[rsl_rl stand-in] iteration 2/2") == 1
    d = torch.load(path, map_location="cpu", weights_only=False)
    assert d["iter"] == 2
    opt = d["optimizer_state_dict"]
    assert len(opt["state"]) == 17 and all(float(s["step"]) == 40.0 for s in opt["state"].values())  # 2 iterations x 5 epochs x 4 mini-batches
    assert opt["param_groups"][0]["lr"] == a["learning_rate"]
    sha = __import__("hashlib").sha256(torch.cat([d["model_state_dict"][n].reshape(-1).float() for n in _parameter_names(d["model_state_dict"])]).numpy().tobytes()).hexdigest()
    assert sha == a["param_sha"], "the checkpoint does not hold the parameters the learner ended with"
    # the second launch: every rank loads the checkpoint through the runner and trains one more iteration
    recs, _ = _launch("train_resume_rank.py", 2, tmp_path, ["--distributed", "--num_envs", "64", "--max_iterations", "1", "--headless"], share, "resume_rank{}.json",
                      RL_TEST_RESUME=path)
    for rec in recs:
        assert rec["learner"] == "HipPPO" and rec["iter_at_load"] == 2 and rec["params_are_the_checkpoint"] and rec["lr_at_load"] == a["learning_rate"]
        assert rec["optimizer_steps"] == [60]
    after = [json.load(open(os.path.join(str(tmp_path), f"rank{r}.json"))) for r in range(2)]  # what the body wrote at the end of the resumed run
    assert all(rec["iterations"] == 3 and rec["finite"] for rec in after)
    assert after[0]["param_sha"] == after[1]["param_sha"] != a["param_sha"] and after[0]["learning_rate"] == after[1]["learning_rate"]
    assert os.path.isfile(os.path.join(str(tmp_path), "logs", "model_3.pt"))


def _parameter_names(state_dict):
    """`ActorCritic.parameters()` order: std, the actor's layers, the critic's"""
    layers = lambda net: sorted({int(k.split(".")[1]) for k in state_dict if k.startswith(net + ".")})  # noqa: E731
    return ["std"] + [f"{net}.{l}.{w}" for net in ("actor", "critic") for l in layers(net) for w in ("weight", "bias")]
