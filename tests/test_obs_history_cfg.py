"""Observation history on the Python surface, no device: the cfg's history_length / flatten_history_dim -> per-term lists
(model/cfg_compile.py compile_obs_history), the row widths they give, the descriptor bundles they must not touch, and the symmetry
tables of a history row (symmetry.expand_history)."""
import json
import os

import numpy as np
import pytest

from robot_lab_amd import shims
from robot_lab_amd.scene import DATA_DIR, load_bundle, save_bundle
from robot_lab_amd.symmetry import expand_history, tables_for_env

A1F = "RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0"
REF = "/root/reference/source/robot_lab"


def _observations(group_hist=None, group_flat=True, term_hist=(0, 0, 0), term_flat=(True, True, True), critic=True):
    """an `observations` cfg container built from the shim's cfg classes, the way the reference's ObservationsCfg is"""
    shims.install()
    from isaaclab.managers import ObservationGroupCfg, ObservationTermCfg

    def base_ang_vel(env):
        return None

    def projected_gravity(env):
        return None

    def joint_pos_rel(env):
        return None

    def group():
        g = ObservationGroupCfg()
        g.history_length, g.flatten_history_dim = group_hist, group_flat
        for name, fn, h, fl in zip(("base_ang_vel", "projected_gravity", "joint_pos"), (base_ang_vel, projected_gravity, joint_pos_rel), term_hist, term_flat):
            t = ObservationTermCfg(func=fn)
            t.history_length, t.flatten_history_dim = h, fl
            setattr(g, name, t)
        g.deleted_term = None  # a term the cfg deleted takes no place in the lists
        return g

    class Observations:
        pass

    o = Observations()
    o.policy = group()
    if critic:
        o.critic = group()
    return o


def test_group_override_against_per_term_values():
    from robot_lab_amd.model.cfg_compile import compile_obs_history

    assert compile_obs_history(_observations()) == {"policy": [0, 0, 0], "critic": [0, 0, 0]}
    assert compile_obs_history(_observations(term_hist=(2, 0, 5))) == {"policy": [2, 0, 5], "critic": [2, 0, 5]}
    # the group's history_length, when not None, replaces every term's - 0 included
    assert compile_obs_history(_observations(group_hist=4, term_hist=(2, 0, 5)))["policy"] == [4, 4, 4]
    assert compile_obs_history(_observations(group_hist=0, term_hist=(2, 0, 5)))["policy"] == [0, 0, 0]
    assert compile_obs_history(_observations(term_hist=(1, 1, 1), critic=False)) == {"policy": [1, 1, 1], "critic": []}
    # ... and its flatten_history_dim then replaces theirs: unflattened terms under a flattened group are fine
    assert compile_obs_history(_observations(group_hist=3, term_flat=(False, False, False)))["policy"] == [3, 3, 3]


def test_unflattened_and_negative_history_are_refused():
    from robot_lab_amd.model.cfg_compile import UnsupportedTerm, compile_obs_history

    with pytest.raises(UnsupportedTerm, match="policy.projected_gravity.*flatten_history_dim=False"):
        compile_obs_history(_observations(term_hist=(0, 2, 0), term_flat=(True, False, True)))
    with pytest.raises(UnsupportedTerm, match="flatten_history_dim=False"):
        compile_obs_history(_observations(group_hist=2, group_flat=False))
    # without history the flag means nothing
    assert compile_obs_history(_observations(term_flat=(False, False, False)))["policy"] == [0, 0, 0]
    assert compile_obs_history(_observations(group_hist=0, group_flat=False))["policy"] == [0, 0, 0]
    with pytest.raises(UnsupportedTerm, match="history_length -1"):
        compile_obs_history(_observations(term_hist=(0, -1, 0)))
    with pytest.raises(UnsupportedTerm, match="history_length -2"):
        compile_obs_history(_observations(group_hist=-2))
    with pytest.raises(UnsupportedTerm, match="exceeds 32"):
        compile_obs_history(_observations(group_hist=33))


def test_row_widths():
    from robot_lab_amd.env import resolve_obs_history

    desc, _ = load_bundle(A1F)
    assert desc.obs_dim(0) == 45 and sum(desc.obs_term_dims(0)) == 45
    for H in (1, 3, 5, 32):
        lists = resolve_obs_history(desc, {"policy": H})
        assert lists == {"policy": [H] * desc.task.n_policy}
        assert desc.obs_dim(0, lists["policy"]) == 45 * H
    assert desc.obs_dim(0, [0] * desc.task.n_policy) == 45  # H = 0: the current frame
    assert desc.obs_dim(0, [3, 0, 1, 3, 2, 0]) == 3 * 3 + 3 + 3 + 3 * 12 + 2 * 12 + 12
    assert resolve_obs_history(desc, None) is None and resolve_obs_history(desc, {}) is None
    with pytest.raises(ValueError, match="lengths for a group of"):
        resolve_obs_history(desc, {"policy": [1, 2]})
    with pytest.raises(ValueError, match="negative"):
        resolve_obs_history(desc, {"critic": -1})
    with pytest.raises(ValueError, match="unknown observation group"):
        resolve_obs_history(desc, {"teacher": 2})


def test_committed_bundle_is_independent_of_the_history(tmp_path):
    """History is not part of the descriptor: a bundle saved from a spec that carries history lists has the bytes of the committed one."""
    desc, extra = load_bundle(A1F)
    blob = json.load(open(os.path.join(DATA_DIR, A1F + ".json")))
    nc = desc.task.n_critic
    for hist in ({"policy": [0] * 6, "critic": [0] * nc}, {"policy": [5] * 6, "critic": [0] * nc}):
        spec = dict(terrain_generator=extra["terrain_generator"], env_spacing=extra["env_spacing"], obs_history=hist,
                    dropped_contact_bodies=blob.get("dropped_contact_bodies"), topology=blob.get("topology"))
        out = tmp_path / "bundle.json"
        save_bundle(str(out), desc, spec)
        assert out.read_bytes() == open(os.path.join(DATA_DIR, A1F + ".json"), "rb").read()


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's cfg classes and URDFs")
def test_edited_reference_cfg_compiles_to_the_lists_and_the_same_descriptor():
    import ctypes

    shims.install(shims.REFERENCE_SOURCE)
    import robot_lab.tasks  # noqa: F401
    from isaaclab_tasks.utils import parse_env_cfg

    from robot_lab_amd.model.cfg_compile import UnsupportedTerm, compile_cfg

    d0, s0 = compile_cfg(parse_env_cfg(A1F, device="cpu", num_envs=8))
    assert s0["obs_history"] == {"policy": [0] * d0.task.n_policy, "critic": [0] * d0.task.n_critic}
    cfg = parse_env_cfg(A1F, device="cpu", num_envs=8)
    cfg.observations.policy.history_length = 5  # the edit people make before a sim-to-real run
    d1, s1 = compile_cfg(cfg)
    assert s1["obs_history"]["policy"] == [5] * d1.task.n_policy and s1["obs_history"]["critic"] == [0] * d1.task.n_critic
    assert d1.obs_dim(0, s1["obs_history"]["policy"]) == 45 * 5
    assert bytes(ctypes.string_at(ctypes.addressof(d0), ctypes.sizeof(d0))) == bytes(ctypes.string_at(ctypes.addressof(d1), ctypes.sizeof(d1)))
    cfg.observations.policy.flatten_history_dim = False
    with pytest.raises(UnsupportedTerm, match="flatten_history_dim=False"):
        compile_cfg(cfg)


class _HistEnv:
    def __init__(self, desc, hist):
        self.desc, self.obs_history = desc, hist


@pytest.mark.parametrize("mirrors", ["lr", "lr,fb"])
def test_mirror_of_a_stack_is_the_stack_of_mirrors(mirrors):
    desc, _ = load_bundle(A1F)
    hist = {"policy": [3, 0, 1, 3, 2, 0], "critic": [2] * desc.task.n_critic}
    frame_tabs, hist_tabs = tables_for_env(desc, mirrors), tables_for_env(_HistEnv(desc, hist), mirrors)
    assert hist_tabs.n_sym == frame_tabs.n_sym == (2 if mirrors == "lr" else 4)
    rng = np.random.default_rng(3)
    for g, name in enumerate(("policy", "critic")):
        dims, H = desc.obs_term_dims(g), [max(1, h) for h in hist[name]]
        fp, fs = frame_tabs.obs if g == 0 else frame_tabs.critic
        hp, hs = hist_tabs.obs if g == 0 else hist_tabs.critic
        assert hp.shape[1] == desc.obs_dim(g, hist[name])
        frames = rng.standard_normal((max(H), 7, sum(dims))).astype(np.float32)  # [time, rows, frame_dim], oldest first

        def stack(fr):  # term-major: the last H_k frames of term k side by side, oldest first
            cols, foff = [], 0
            for d, h in zip(dims, H):
                cols += [fr[len(fr) - h + s][:, foff:foff + d] for s in range(h)]
                foff += d
            return np.concatenate(cols, axis=1)

        for s in range(hist_tabs.n_sym):
            mirrored_frames = [fs[s] * f[:, fp[s]] for f in frames]
            row = stack(frames)
            assert np.array_equal(hs[s] * row[:, hp[s]], stack(mirrored_frames))
    # the action table is untouched, a group without history keeps its per-frame table
    assert np.array_equal(hist_tabs.act[0], frame_tabs.act[0])
    only_policy = tables_for_env(_HistEnv(desc, {"policy": [2] * 6}), mirrors)
    assert np.array_equal(only_policy.critic[0], frame_tabs.critic[0]) and only_policy.obs[0].shape[1] == 90


def test_a_permutation_across_term_blocks_is_refused():
    perm = np.array([[0, 1, 2, 3, 4, 5], [0, 1, 3, 2, 4, 5]])  # copy 1 swaps the last column of term 0 with the first of term 1
    sign = np.ones_like(perm, dtype=np.float32)
    with pytest.raises(ValueError, match="crosses term blocks"):
        expand_history((perm, sign), [3, 3], [2, 2])
    p, s = expand_history((perm, sign), [2, 2, 2], [2, 0, 1])  # the same swap inside ONE term: fine
    assert p.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 5, 4, 6, 7]] and s.shape == p.shape
    with pytest.raises(ValueError, match="history lengths for"):
        expand_history((perm, sign), [3, 3], [2])
    with pytest.raises(ValueError, match="add up to"):
        expand_history((perm, sign), [3, 4], [2, 2])
