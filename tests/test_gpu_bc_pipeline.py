"""The BC update step's host pipeline: run-ahead (update_parameters(sync=False)), prefetch into the second input / geometry set,
the step as one replayed launch list with one fused optimiser launch -- against the synchronous loop and against the same list
walked call by call from Python (runtime.STEP_PLAN = False, set_fused_optim(False), engine.SERIAL)."""
import contextlib
import functools
import random

import numpy as np
import pytest
import torch

from tests import test_gpu_step as tstep
from tests.helpers import assert_close
from tests.test_gpu_deterministic import _assert_bitwise, _mode, _schedule, _state

pytestmark = pytest.mark.gpu
CFG = "bc_dagger_aux.yaml"


@contextlib.contextmanager
def _step_plan(on):
    from ga_ddpg_amd import runtime
    saved = runtime.STEP_PLAN
    runtime.STEP_PLAN = bool(on)
    try:
        yield
    finally:
        runtime.STEP_PLAN = saved


@functools.lru_cache(maxsize=None)
def _memory():
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    cfg = load_cfg(CFG)
    mem = BaseMemory(1500, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(mem, 1500, seed=5)
    return mem, cfg


def _valid_indices(mem, B, n, seed):
    """index vectors of minibatches with at least one expert, one positive-return and one unperturbed row (synth_data.sample_valid_batch's
    rule: the reference's masked means are NaN otherwise)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        idx = mem.draw_indices(B, rng)
        if (mem.expert_flags[idx] >= 1).any() and (mem.returns[idx] > 0).any() and (mem.perturb_flags[idx] < 1).any():
            out.append(np.asarray(idx))
    return out


def _zero_lr(agent):
    for opt in (agent.policy_optim, agent.state_feat_encoder_optim, agent.state_feat_val_encoder_optim):
        for g in opt.param_groups:
            g["lr"] = 0.0


def _assert_logs_close(got, want, what):
    assert len(got) == len(want)
    for s, (a, b) in enumerate(zip(want, got)):
        assert set(a.keys()) == set(b.keys()) and len(a) == 11
        for k in a:
            assert_close(b[k], a[k], 2e-4, 1e-6, "%s step %d %s" % (what, s, k))


@pytest.mark.parametrize("source", ["host", "device"])
def test_bc_run_ahead_steps_equal_synchronous_steps(source):
    """seven steps (more than staging sets) at learning rate 0: every step's numbers depend on ITS minibatch only, so a step that
    read another step's inputs, geometry or staging block shows up against the synchronous loop"""
    from ga_ddpg_amd.core.agent import PendingLog
    from ga_ddpg_amd.runtime import BATCH_KEYS
    mem, _ = _memory()
    batches = [mem.sample(32, batch_idx=i) for i in _valid_indices(mem, 32, 7, 3)]
    if source == "device":
        batches = [{k: torch.as_tensor(np.ascontiguousarray(b[k], dtype=np.float32)).cuda() for k in BATCH_KEYS} for b in batches]

    def run(mode):
        agent, nets = tstep._filled_agent(CFG, 11)
        _zero_lr(agent)
        logs = []
        for i, b in enumerate(batches):
            if mode == "prefetch" and i + 1 < len(batches):
                staged = agent.prefetch(batches[i + 1])      # no runtime before the first step; host batches are never staged ahead
                assert staged == (source == "device" and i >= 1), (i, staged)
            out = agent.update_parameters(b, agent.update_step, 0, sync=(mode != "ahead"))
            agent.step_scheduler(agent.update_step)
            logs.append(out)
        assert agent.pi is agent._rt.pi and agent.aux_pred is agent._rt.aux_pred
        if mode == "ahead":
            assert all(isinstance(l, PendingLog) for l in logs)
            assert not logs[-1].done()                       # nothing was read yet
            agent.flush()
        return [dict(l) for l in logs]
    sync = run("sync")
    assert abs(sync[2]["bc_loss"] - sync[3]["bc_loss"]) > 1e-4            # the batches do differ
    _assert_logs_close(run("ahead"), sync, "run-ahead")
    _assert_logs_close(run("prefetch"), sync, "prefetched")


# ------------------------------------------------------------------------------------------------ deterministic mode: bit equality
DET_B, DET_STEPS = 64, 6
NEW_LR = 2.5e-4


@functools.lru_cache(maxsize=None)
def _det_run(path, lr_change=False):
    """six BC steps at B = 64 over the HBM mirror of the synthetic buffer, the same batch_idx on every path -> every tensor the steps
    wrote (tests.test_gpu_deterministic._state).  Call inside _mode()."""
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    mem, _ = _memory()
    idx = _valid_indices(mem, DET_B, DET_STEPS, 77)
    random.seed(91)
    np.random.seed(91)
    torch.manual_seed(91)
    dmem = DeviceReplay(mem)
    agent, nets = tstep._filled_agent(CFG, 91)
    ahead = path == "run_ahead"
    draw = (lambda i: dmem.sample_lazy(DET_B, batch_idx=idx[i])) if ahead else (lambda i: dmem.sample(DET_B, batch_idx=idx[i]))
    rt = agent.runtime(DET_B, int(dmem.point_state.shape[2]))
    if path == "unfused":
        rt.set_fused_optim(False)
    results = []
    with _schedule("serial" if path == "serial" else "default"), _step_plan(path != "no_step_plan"):
        assert rt._replays() == (path in ("default", "run_ahead"))
        nxt = draw(0)
        for i in range(DET_STEPS):
            if lr_change and i == 2:
                agent.policy_optim.param_groups[0]["lr"] = NEW_LR
                agent.state_feat_encoder_optim.param_groups[0]["lr"] = NEW_LR
            cur, nxt = nxt, (draw(i + 1) if i + 1 < DET_STEPS else None)
            if ahead and nxt is not None:
                agent.prefetch(nxt)
            results.append(agent.update_parameters(cur, agent.update_step, i, sync=not ahead))
            agent.step_scheduler(agent.update_step)
        agent.flush()
        torch.cuda.synchronize()
    results = [{k: float(v) for k, v in r.items()} for r in results]
    return _state(agent, nets, results)


@pytest.mark.parametrize("path", ["no_step_plan", "unfused", "serial", "run_ahead"])
def test_det_bc_paths_bitwise(path):
    """the replayed list with the fused optimiser launch (default) against: the same launches call by call; the separate Adam /
    target / statistics launches; one stream; run-ahead with prefetch over sample_lazy handles -- parameters, policy_target,
    running statistics and num_batches_tracked, both Adam moments and the logs agree bit for bit"""
    with _mode():
        ref = _det_run("default")
        assert len(ref) > 100 and any(k.endswith("num_batches_tracked") for k in ref)
        _assert_bitwise(ref, _det_run(path), path)


def test_det_bc_learning_rate_change_reaches_the_right_step_under_run_ahead():
    """the Adam scalars are read from the torch optimisers at enqueue time: a learning rate set between two enqueued steps acts from
    the following step on, as in the synchronous loop"""
    with _mode():
        ref = _det_run("default", True)
        _assert_bitwise(ref, _det_run("run_ahead", True), "run-ahead with a learning-rate change")
        base = _det_run("default")
        assert any(not torch.equal(ref[k], base[k]) for k in ref if k.startswith("policy/"))      # the new rate did act


# ------------------------------------------------------------------------------------------------ staging safety
def test_bc_prefetch_sampler_under_run_ahead_steps():
    """run-ahead updates return before their uploads have run: a PrefetchSampler staging set must not be refilled until the event
    the runtime hangs on the batch (`uploaded_event`)"""
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    from ga_ddpg_amd.synth_data import sample_valid_batch
    mem, _ = _memory()
    runs = {}
    for mode in ("sync", "ahead"):
        agent, _nets = tstep._filled_agent(CFG, 5)
        _zero_lr(agent)
        rng = np.random.default_rng(2)
        logs = []
        with PrefetchSampler(mem, 32, depth=1, sample=lambda n: sample_valid_batch(mem, n, rng)) as s:   # two staging sets circulate
            for i in range(10):
                logs.append(agent.update_parameters(s.next(), agent.update_step, i, sync=(mode == "sync")))
            agent.flush()
        runs[mode] = [dict(l) for l in logs]
    _assert_logs_close(runs["ahead"], runs["sync"], "PrefetchSampler run-ahead")
    assert abs(runs["sync"][0]["bc_loss"] - runs["sync"][1]["bc_loss"]) > 1e-4


# ------------------------------------------------------------------------------------------------ the kept path under the parity gates
def test_call_by_call_bc_step_vs_reference_golden(golden_dir):
    with _step_plan(False):
        tstep.test_bc_steps_vs_reference_golden(golden_dir)


def test_call_by_call_bc_step_config0_batch64_vs_oracle():
    with _step_plan(False):
        tstep.test_bc_step_config0_batch64_vs_oracle()


# ------------------------------------------------------------------------------------------------ the driver
def test_train_off_policy_bc_loops_bitwise(monkeypatch, tmp_path):
    """train_off_policy over the HBM mirror, B = 32, five updates per epoch, two epochs: the plain loop, the default lookahead loop
    and run_ahead=True give the same loss history and parameters in deterministic mode; a checkpoint carries the step count"""
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.experiments.config import load_cfg
    mem, _ = _memory()

    def run(loop):
        monkeypatch.setenv("GAD_TRAIN_LOOKAHEAD", "0" if loop == "plain" else "1")
        config = load_cfg(CFG).RL_TRAIN
        config.batch_size, config.updates_per_step = 32, 5
        assert config.max_epoch > 100
        agent, nets = tstep._filled_agent(CFG, 17)
        losses, epochs = tto.train_off_policy(agent, mem, config, max_epochs=2, run_ahead=(loop == "run_ahead"), device_replay=True,
                                              rng=np.random.default_rng(4))
        assert epochs == 2 and agent.update_step == 11
        hist = {k: np.asarray(list(h), dtype=np.float64) for k, h in losses.items()}
        assert len(hist["bc_loss"]) == 11 and np.isfinite(hist["bc_loss"]).all()      # deque([0]) + 10 updates
        return agent, hist, _state(agent, nets, [])
    with _mode():
        agent, hist, state = run("plain")
        for loop in ("lookahead", "run_ahead"):
            _, h, s = run(loop)
            assert all(h[k].tobytes() == hist[k].tobytes() for k in hist), loop
            _assert_bitwise(state, s, loop)
        agent.save_model(agent.update_step, output_dir=str(tmp_path))
        fresh, _nets = tstep._filled_agent(CFG, 18)
        fresh.load_model(str(tmp_path))
        counters = {k: int(v) for k, v in fresh.state_feature_extractor.state_dict().items()
                    if k.endswith("num_batches_tracked") and "value_encoder" not in k}
        assert counters and set(counters.values()) == {10}, counters
