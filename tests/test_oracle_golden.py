"""The CPU oracle (oracle/ref_step.py) against golden vectors produced by the reference's own
Python (oracle/make_golden.py).  Float tolerance: 2e-5 relative (same torch kernels, same order;
the only slack is summation order inside torch)."""
import json
import os

import numpy as np
import pytest
import torch

from ga_ddpg_amd.experiments.config import load_cfg
from oracle import ref_step
from oracle.detfill import fill_module_
from tests.helpers import assert_close, check_summaries, golden_batch

RT, AT = 2e-5, 1e-7
SEED = 1234


def _agent(cfg_name, seed):
    torch.manual_seed(0)
    c = load_cfg(cfg_name)
    a = ref_step.OracleAgent(c.RL_TRAIN)
    for name, net in a.nets().items():
        fill_module_(net, name, seed)
    return a


def test_losses_and_noise(golden_dir):
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    pred = torch.tensor(g["goal_pred"], requires_grad=True)
    l = ref_step.goal_pred_loss(pred, torch.tensor(g["goal_gt"]))
    l.backward()
    assert_close(l.item(), g["goal_loss"], RT, AT, "goal loss")
    assert_close(pred.grad.numpy(), g["goal_grad"], RT, 1e-7, "goal grad")
    pi = torch.tensor(g["bc_pi"], requires_grad=True)
    l2 = ref_step.pose_bc_loss(pi, torch.tensor(g["bc_act"]))
    l2.backward()
    assert_close(l2.item(), g["bc_loss"], RT, AT, "bc loss")
    assert_close(pi.grad.numpy(), g["bc_grad"], RT, 1e-7, "bc grad")
    d = ref_step.target_noise(torch.tensor(g["noise_u"]).clone(), float(g["noise_level"]))
    assert_close(d.numpy(), g["noise_delta"], 1e-6, 0, "noise")
    # the reference's quirk: (u*3-6)*level is always negative -> translation noise clamps to -0.01
    assert (g["noise_delta"] < 0).all()


def test_float64_loss_references_reproduce_golden(golden_dir):
    """The yardstick of tests/test_gpu_head_losses.py: goal_pred_loss, pose_bc_loss and target_noise evaluated in float64 on
    the golden inputs reproduce the reference's own float32 results (core/loss.py, core/utils.py get_noise_delta) to float32
    rounding: 4 ulp (2.4e-7) of the value for the losses and noise, of the tensor's max for the gradients."""
    f32 = 2.0 ** -22
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    d64 = lambda k: torch.tensor(g[k], dtype=torch.float64)
    pred = d64("goal_pred").requires_grad_(True)
    l = ref_step.goal_pred_loss(pred, d64("goal_gt"))
    l.backward()
    assert_close(l.item(), g["goal_loss"], f32, 0, "goal loss (float64)")
    assert_close(pred.grad.numpy(), g["goal_grad"], 0, f32 * np.abs(pred.grad.numpy()).max(), "goal grad (float64)")
    pi = d64("bc_pi").requires_grad_(True)
    l2 = ref_step.pose_bc_loss(pi, d64("bc_act"))
    l2.backward()
    assert_close(l2.item(), g["bc_loss"], f32, 0, "bc loss (float64)")
    assert_close(pi.grad.numpy(), g["bc_grad"], 0, f32 * np.abs(pi.grad.numpy()).max(), "bc grad (float64)")
    d = ref_step.target_noise(d64("noise_u").clone(), float(g["noise_level"]))
    assert_close(d.numpy(), g["noise_delta"], f32, 0, "noise (float64)")


def test_heads(golden_dir):
    g = np.load(os.path.join(golden_dir, "heads.npz"))
    x = torch.tensor(g["x"])
    q = fill_module_(ref_step.QNet(513, 256, 7), "critic", SEED)
    q1, q2, aux = q(x)
    assert_close(q1.detach().numpy(), g["q1"], RT, 1e-6, "q1")
    assert_close(q2.detach().numpy(), g["q2"], RT, 1e-6, "q2")
    assert_close(aux.detach().numpy(), g["aux"], RT, 1e-6, "aux")
    p = fill_module_(ref_step.PolicyNet(513, 6, 256, 7), "policy", SEED)
    pi, extra = p(x)
    assert_close(pi.detach().numpy(), g["pi_mean"], RT, 1e-7, "pi")
    assert_close(extra.detach().numpy(), g["pi_extra"], RT, 1e-6, "pi extra")
    # GaussianPolicy.forward / sample with the injected rsample draw (reference core/networks.py:339-371)
    for tag, dim in (("pi", 7), ("p1", 1)):
        p = fill_module_(ref_step.PolicyNet(513, 6, 256, dim), "policy", SEED)
        msq, logp, act, extra, mean, log_std = [t.detach().numpy() for t in p.sample(x, torch.tensor(g["pi_eps"]))]
        assert_close(msq, g[tag + "_mean"], RT, 1e-7, tag + " squashed mean")
        assert_close(logp, g[tag + "_log_prob"], 1e-5, 1e-5, tag + " log_prob")
        assert_close(act, g[tag + "_action"], RT, 1e-7, tag + " action")
        assert_close(extra, g[tag + "_extra"], RT, 1e-6, tag + " extra")
        if tag == "pi":
            assert_close(mean, g["pi_raw_mean"], RT, 1e-6, "raw mean")
            assert_close(log_std, g["pi_log_std"], RT, 1e-6, "log_std")


def test_encoder_forward_backward(golden_dir):
    g = np.load(os.path.join(golden_dir, "encoder_B16.npz"))
    net = ref_step.PointFeature(extra_latent=1, action_concat=True)
    shell = fill_module_(ref_step._DataParallelShell(net), "state_feature_extractor", SEED)
    shell.train()
    pc = torch.tensor(g["point_state"])
    act = torch.tensor(g["action"], requires_grad=True)
    z_pol = net(pc, value=False)
    pc10 = torch.cat((pc, act.unsqueeze(2).expand(-1, -1, pc.shape[2])), 1)
    z_val = net(pc10, value=True)
    probe = torch.tensor(g["probe"])
    ((z_pol * probe).sum() + (z_val * probe.flip(1)).sum()).backward()
    assert_close(z_pol.detach().numpy(), g["z_policy"], RT, 1e-6, "z_policy")
    assert_close(z_val.detach().numpy(), g["z_value"], RT, 1e-6, "z_value")
    assert_close(act.grad.numpy(), g["action_grad"], 1e-4, 1e-6, "action grad")
    check_summaries(g, "grad/", ((n, q.grad) for n, q in net.named_parameters()), 1e-4, 1e-6)
    check_summaries(g, "state/", net.state_dict().items(), RT, 1e-6)


def _check_step(a, g, p, kind, test=False):
    batch = golden_batch(g, p)
    if test:
        ret = a.update_parameters(batch, noise_u=g[p + "noise_u"], test=True)
    else:
        ret = a.update_parameters(batch, noise_u=g[p + "noise_u"] if kind == "ddpg" else None)
    a.step_scheduler()
    for k, v in ret.items():
        assert_close(v, g[p + "ret/" + k], 1e-4, 1e-6, p + k)
    d = a.dbg
    assert_close(d["pi"].numpy(), g[p + "t/pi"], 1e-4, 1e-6, p + "pi")
    assert_close(d["aux_pred"].numpy(), g[p + "t/aux_pred"], 1e-4, 1e-6, p + "aux_pred")
    if kind == "ddpg":
        for mine, theirs in (("value_feat", "feat0"), ("next_state", "feat1"), ("next_target", "feat2"),
                             ("policy_feat", "feat3")):
            assert_close(d[mine].numpy(), g[p + theirs], 1e-4, 1e-6, p + mine)
        assert_close(d["q1"].numpy(), g[p + "t/qf1"], 1e-4, 1e-6, p + "qf1")
        assert_close(d["q2"].numpy(), g[p + "t/qf2"], 1e-4, 1e-6, p + "qf2")
        assert_close(d["y"].numpy(), g[p + "t/next_q_value"], 1e-4, 1e-6, p + "y")
        if p + "t/qf1_pi" in g.files:
            assert_close(d["q1_pi"].numpy(), g[p + "t/qf1_pi"], 1e-4, 1e-6, p + "qf1_pi")
    nets = a.nets()
    # FC-layer biases in front of a train-mode BatchNorm have an analytically zero gradient; what
    # the reference holds there is float noise (1e-9) which Adam then amplifies -> excluded.
    skip = (".1.0.bias", ".1.3.bias")
    for name in (["policy", "state_feature_extractor"] + (["critic"] if kind == "ddpg" else [])):
        check_summaries(g, p + "end/grad/" + name + "/", ((n, q.grad) for n, q in nets[name].named_parameters()),
                        2e-4, 1e-7, skip=skip)
    for name, net in nets.items():
        check_summaries(g, p + "end/param/" + name + "/", net.state_dict().items(), 1e-4, 2e-6, skip=skip)


def test_ddpg_steps(golden_dir):
    g = np.load(os.path.join(golden_dir, "ddpg_steps_B32.npz"))
    for run, start, nsteps in (("a", 1, 1), ("b", 2, 2)):
        a = _agent("ddpg_td3_aux.yaml", SEED)
        a.update_step = start
        for s in range(nsteps):
            assert a.update_step == int(g["%s%d/update_step" % (run, s)])
            _check_step(a, g, "%s%d/" % (run, s), "ddpg")
    assert "b0/t/qf1_pi" in g.files and "a0/t/qf1_pi" not in g.files     # b0 is the policy-update step


def test_ddpg_steps_test_mode(golden_dir):
    """update_parameters(test=True) as the reference's own classes run it (eval-mode BatchNorm in every pass, forward and
    backward; tests/golden/ddpg_steps_test_mode_B32.npz from oracle/make_golden.py): the oracle reproduces it, and the running
    statistics / batch counters stay where they were"""
    from oracle.detfill import fill_running_stats_
    g = np.load(os.path.join(golden_dir, "ddpg_steps_test_mode_B32.npz"))
    for run, start in (("e", 1), ("f", 2)):
        a = _agent("ddpg_td3_aux.yaml", SEED)
        for name, net in a.nets().items():
            fill_running_stats_(net, name, SEED)
        before = {k: v.clone() for k, v in a.state_feature_extractor.state_dict().items() if "running" in k or "num_batches" in k}
        a.update_step = start
        assert a.update_step == int(g["%s0/update_step" % run])
        _check_step(a, g, "%s0/" % run, "ddpg", test=True)
        for k, v in a.state_feature_extractor.state_dict().items():
            if k in before:
                assert torch.equal(v, before[k]), k
    assert "f0/t/qf1_pi" in g.files and "e0/t/qf1_pi" not in g.files


def test_ddpg_step_asymmetric_action_bounds(golden_dir):
    """an action space with asymmetric bounds (action_bias = (high + low) / 2 != 0, core/networks.py:329-337): the reference's own
    policy step (tests/golden/ddpg_steps_asym_bounds_B32.npz) reproduced by the oracle"""
    from oracle.detfill import AsymTaskSpace6D
    g = np.load(os.path.join(golden_dir, "ddpg_steps_asym_bounds_B32.npz"))
    a = _agent("ddpg_td3_aux.yaml", SEED)
    for pol in (a.policy, a.policy_target):
        pol.set_action_space(AsymTaskSpace6D())
    assert_close(a.policy.action_bias.numpy(), g["g0/action_bias"], 1e-7, 0, "action_bias")
    a.update_step = 2
    _check_step(a, g, "g0/", "ddpg")


def test_bc_steps(golden_dir):
    g = np.load(os.path.join(golden_dir, "bc_steps_B32.npz"))
    a = _agent("bc_dagger_aux.yaml", SEED + 1)
    for s in range(2):
        _check_step(a, g, "a%d/" % s, "bc")


def test_config_matches_reference(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "config_rl_train.json")))
    for mine, want in ref.items():
        c = load_cfg(mine)
        for k, v in want["top"].items():
            assert c[k] == v, (mine, k, c[k], v)
        for k, v in want["RL_TRAIN"].items():
            if k == "index_file":
                continue
            got = c.RL_TRAIN[k]
            assert (list(got) == list(v)) if isinstance(v, list) else (got == v), (mine, k, got, v)
        assert set(c.RL_TRAIN.keys()) == set(want["RL_TRAIN"].keys())


def test_replay_sample_matches_reference(golden_dir):
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    g = np.load(os.path.join(golden_dir, "replay_sample.npz"))
    c = load_cfg("ddpg_td3_aux.yaml")
    c.RL_TRAIN.uniform_num_pts = 64
    mem = BaseMemory(400, c)
    for k in ("action", "expert_action", "point_state", "reward", "terminal", "timestep", "returns", "goal",
              "episode_map", "expert_flags", "perturb_flags"):
        getattr(mem, k)[...] = g["buffer/" + k]
    mem.cur_idx = int(g["buffer/cur_idx"])
    mem.state_pose[:] = np.eye(4, dtype=np.float32)   # what fill_synthetic_buffer stores
    np.random.seed(SEED)
    data = mem.sample(16)
    keys = [k[len("batch/"):] for k in g.files if k.startswith("batch/")]
    assert set(keys) == set(data.keys()) and len(keys) == 22
    for k in keys:
        assert data[k].dtype == g["batch/" + k].dtype, k
        np.testing.assert_array_equal(data[k], g["batch/" + k], err_msg=k)
    mem.recompute_return_with_gamma()
    np.testing.assert_array_equal(mem.returns, g["recomputed_returns"])


def _replay_episodes(n_pts, seed):
    """the seeded rollouts oracle/make_golden.py::_episodes fed to the reference's add_episode"""
    rng = np.random.default_rng(seed)
    eps = []
    for e in range(7):
        L = int(rng.integers(3, 9))
        success = bool(e % 3 != 1)
        ep = []
        for t in range(L):
            cloud = rng.normal(size=(4, n_pts + 6)) * 0.1
            if e == 4 and t == 2:
                cloud[:] = 0.0
            ep.append({"point_state": cloud, "action": rng.normal(size=6).astype(np.float32),
                       "expert_action": rng.normal(size=6).astype(np.float32), "goal": rng.normal(size=7).astype(np.float32),
                       "reward": np.float32(1.0 if (success and t == L - 1) else 0.0), "terminal": np.float32(t == L - 1),
                       "timestep": np.float32(t), "expert_flags": np.float32(e % 2), "perturb_flags": np.float32(t == 1),
                       "state_pose": np.eye(4, dtype=np.float32), "target_idx": np.float32(e), "target_name": "obj%d" % (e % 3)})
        eps.append(ep)
    return eps


def test_replay_writer_and_disk_format_match_reference(golden_dir, tmp_path):
    """add_episode (return back-fill, episode_map, dropped frames), save, load and sample-after-load
    against the reference's own BaseMemory (tests/golden/replay_io.npz; replay_io_saved.npz is the file the REFERENCE
    wrote -- we must load it, and the file we write must hold the same arrays)."""
    import shutil
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    g = np.load(os.path.join(golden_dir, "replay_io.npz"))
    c = load_cfg("ddpg_td3_aux.yaml")
    c.RL_TRAIN.uniform_num_pts = 128
    c.RL_SAVE_DATA_NAME = "replay_io_saved.npz"
    mem = BaseMemory(48, c)
    for ep in _replay_episodes(128, SEED + 9):
        mem.add_episode(ep)
    for k in ("action", "reward", "returns", "terminal", "timestep", "episode_map", "expert_flags", "perturb_flags", "goal"):
        np.testing.assert_array_equal(getattr(mem, k), g["after_add/" + k], err_msg=k)
    assert (mem.cur_idx, mem.total_env_step, mem.is_full) == (int(g["after_add/cur_idx"]), int(g["after_add/total_env_step"]),
                                                              bool(g["after_add/is_full"]))
    # our file == the reference's file, array by array
    mem.save(str(tmp_path))
    ours, theirs = np.load(tmp_path / "replay_io_saved.npz", allow_pickle=True), np.load(
        os.path.join(golden_dir, "replay_io_saved.npz"), allow_pickle=True)
    assert sorted(ours.files) == sorted(theirs.files)
    for k in theirs.files:
        np.testing.assert_array_equal(ours[k], theirs[k], err_msg="saved " + k)
    # load the reference's file into a fresh buffer, then sample like the reference did
    d = tmp_path / "in"
    d.mkdir()
    shutil.copy(os.path.join(golden_dir, "replay_io_saved.npz"), d / "replay_io_saved.npz")
    mem2 = BaseMemory(48, c)
    mem2.load(str(d))
    assert mem2.cur_idx == int(g["after_load/cur_idx"])
    np.testing.assert_array_equal(mem2.returns, g["after_load/returns"])
    assert float(mem2.point_state.sum()) == float(g["after_load/point_state_sum"])
    np.random.seed(SEED + 1)
    mem2.episode_max_len = 2
    data = mem2.sample(8)
    for k in [k[len("batch/"):] for k in g.files if k.startswith("batch/")]:
        np.testing.assert_array_equal(data[k], g["batch/" + k], err_msg=k)
    mem3 = BaseMemory(48, c)
    mem3.load(str(tmp_path / "does_not_exist"))            # silently ignored, like the reference
    assert mem3.cur_idx == 0
