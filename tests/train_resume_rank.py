"""Test infrastructure: ONE rank of a RESUMED run.  The body is tests/train_body_rank.py itself (the reference's `train.py --distributed`, call for
call; one copy of the agent cfg); what `train.py --resume` adds - `runner.load(resume_path)` between the runner's construction and `learn()`
(train.py:214-216) - is put in front of the runner's `learn`.  The checkpoint is `$RL_TEST_RESUME`; beside the body's `$RL_TEST_OUT/rank<r>.json`
this writes `$RL_TEST_OUT/resume_rank<r>.json`: what the runner held after the load and after the resumed iterations.  The learner is the runner's
choice (`RL_LEARNER`)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from robot_lab_amd import shims

    shims.install()
    import torch
    import train_body_rank
    from rsl_rl.runners import OnPolicyRunner

    learn = OnPolicyRunner.learn

    def load_then_learn(runner, *a, **k):
        path = os.environ["RL_TEST_RESUME"]
        runner.load(path)  # every rank loads the one checkpoint rank 0 wrote
        loaded = torch.load(path, map_location="cpu", weights_only=False)
        flat = torch.cat([p.detach().reshape(-1).float().cpu() for p in runner.alg.policy.parameters()])
        want = torch.cat([loaded["model_state_dict"][n].reshape(-1).float() for n, _ in runner.alg.policy.named_parameters()])
        rec = dict(iter_at_load=runner.current_learning_iteration, lr_at_load=float(runner.alg.learning_rate), params_are_the_checkpoint=bool(torch.equal(flat, want)))
        learn(runner, *a, **k)
        opt = runner.alg.optimizer_state_dict() if hasattr(runner.alg, "optimizer_state_dict") else runner.alg.optimizer.state_dict()
        rec.update(learner=type(runner.alg).__name__, optimizer_steps=sorted({int(float(s["step"])) for s in opt["state"].values()}))
        with open(os.path.join(os.environ["RL_TEST_OUT"], f"resume_rank{os.environ.get('RANK', '0')}.json"), "w") as f:
            json.dump(rec, f)

    OnPolicyRunner.learn = load_then_learn
    train_body_rank.main()


if __name__ == "__main__":
    main()
