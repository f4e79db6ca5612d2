"""Deterministic mode (library option "deterministic", torch.use_deterministic_algorithms): update steps that are bit-identical
whatever the schedule -- stream interleaving, grid-rows hints, run-ahead -- and façade backward ops that do not depend on the
order of colliding additions.  Parity with the reference in the mode goes through the helpers of tests/test_gpu_step.py."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from ga_ddpg_amd import hip
from tests import test_gpu_step as tstep

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _mode(on=True):
    prev = hip.get_option("deterministic")
    hip.set_option("deterministic", int(on))
    try:
        yield
    finally:
        hip.set_option("deterministic", prev)


@contextlib.contextmanager
def _schedule(name):
    from ga_ddpg_amd import engine, runtime
    saved = (engine.SERIAL, runtime.ROW_HINTS)
    engine.SERIAL = name == "serial"
    runtime.ROW_HINTS = name != "no_row_hints"
    try:
        yield
    finally:
        engine.SERIAL, runtime.ROW_HINTS = saved


def _memory(cfg_name, seed):
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    mem = BaseMemory(1500, load_cfg(cfg_name), point_dtype=np.float32)
    fill_synthetic_buffer(mem, 1500, seed=seed)
    return mem


def _state(agent, nets, results):
    """every tensor a step writes: parameters and buffers of all networks (targets, running statistics), Adam moments"""
    out = {"res/%d/%s" % (i, k): torch.tensor(float(v), dtype=torch.float64) for i, r in enumerate(results) for k, v in r.items()}
    for name, net in nets.items():
        for k, v in net.state_dict().items():
            out[name + "/" + k] = v.detach().cpu().clone()
    agent._optim_states_out()
    for oname in ("policy_optim", "critic_optim", "state_feat_encoder_optim", "state_feat_val_encoder_optim"):
        opt = getattr(agent, oname, None)
        if opt is None:
            continue
        for i, p in enumerate(p for grp in opt.param_groups for p in grp["params"]):
            st = opt.state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    out["%s/%d/%s" % (oname, i, k)] = st[k].detach().cpu().clone()
    return out


def _run_steps(cfg_name, kind, B, schedule, nsteps=6, seed=91, before_step=None):
    """before_step(agent, i, batch): called in front of step i (switches a test flips between steps)"""
    import random
    from ga_ddpg_amd.synth_data import sample_valid_batch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)                      # (the step's own random draws: every run starts from the same generator state)
    mem = _memory(cfg_name, 6)
    rng = np.random.default_rng(77)
    batches = [sample_valid_batch(mem, B, rng) for _ in range(nsteps)]
    noise = [rng.random((B, 6)).astype(np.float32) for _ in range(nsteps)]
    agent, nets = tstep._filled_agent(cfg_name, seed)
    if kind == "ddpg":
        agent.update_step = 1
    results = []
    with _schedule(schedule):
        for i in range(nsteps):
            if before_step is not None:
                before_step(agent, i, batches[i])
            if kind == "bc":
                results.append(agent.update_parameters(batches[i], agent.update_step, i))
            elif schedule == "run_ahead":
                results.append(agent.update_parameters(batches[i], agent.update_step, i, noise_u=noise[i], sync=False))
                if i + 1 < nsteps:
                    agent.prefetch(batches[i + 1])
            else:
                results.append(agent.update_parameters(batches[i], agent.update_step, i, noise_u=noise[i]))
            agent.step_scheduler(agent.update_step)
        if hasattr(agent, "flush"):
            agent.flush()
        torch.cuda.synchronize()
    results = [{k: float(v) for k, v in r.items()} for r in results]
    return _state(agent, nets, results)


def _assert_bitwise(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, "%s: %d of %d tensors differ, e.g. %s" % (what, len(bad), len(a), bad[:8])


def test_det_ddpg_steps_bitwise_across_schedules():
    """B = 256, N = 1024 (the bench shape), six steps crossing policy and non-policy updates: the default schedule, one stream
    (engine.SERIAL), no grid-rows hints and run-ahead with prefetch give the same bits everywhere"""
    with _mode():
        ref = _run_steps("ddpg_td3_aux.yaml", "ddpg", 256, "default")
        assert len(ref) > 100
        for sched in ("serial", "no_row_hints", "run_ahead"):
            _assert_bitwise(ref, _run_steps("ddpg_td3_aux.yaml", "ddpg", 256, sched), sched)


def test_det_bc_steps_bitwise_across_schedules():
    with _mode():
        ref = _run_steps("bc_dagger_aux.yaml", "bc", 64, "default", nsteps=4)
        for sched in ("serial", "no_row_hints"):
            _assert_bitwise(ref, _run_steps("bc_dagger_aux.yaml", "bc", 64, sched, nsteps=4), sched)


# ------------------------------------------------------------------------------------------------ one list, two ways to run it
@contextlib.contextmanager
def _path(name):
    """no_step_plan: the step's launch list walked item by item from Python (runtime.STEP_PLAN off); plan_py: every plan walked
    (engine.USE_C_PLANS off); unfused is a property of the runtime (_unfused_from_step_0)"""
    from ga_ddpg_amd import engine, runtime
    saved = (runtime.STEP_PLAN, engine.USE_C_PLANS)
    runtime.STEP_PLAN = name != "no_step_plan"
    engine.USE_C_PLANS = name != "plan_py"
    try:
        yield
    finally:
        runtime.STEP_PLAN, engine.USE_C_PLANS = saved


def _unfused_from_step_0(agent, i, batch):
    if i == 0:
        ps = batch["point_state_batch"]
        agent.runtime(ps.shape[0], ps.shape[2]).set_fused_optim(False)


PATH_B, PATH_STEPS = 32, 4


@functools.lru_cache(maxsize=None)
def _ddpg_path_run(path):
    """four DDPG steps at B = 32 from update_step = 1 with injected noise -> (_state, [was step i a policy step]).  Call inside _mode()."""
    kinds = []

    def before(agent, i, batch):
        kinds.append(agent.update_step % agent.policy_update_gap == 0)
        if path == "unfused":
            _unfused_from_step_0(agent, i, batch)
    with _path(path):
        state = _run_steps("ddpg_td3_aux.yaml", "ddpg", PATH_B, "default", nsteps=PATH_STEPS, before_step=before)
    return state, tuple(kinds)


@pytest.mark.parametrize("path", ["no_step_plan", "unfused", "plan_py"])
def test_det_ddpg_paths_bitwise(path):
    """the replayed list with the fused optimiser launches (default) against: the same list walked from Python; the separate
    gad_sumsq / Adam / target / statistics launches; every plan walked instead of replayed in C -- two policy and two non-policy
    steps, every tensor the steps wrote and the logs agree bit for bit"""
    with _mode():
        ref, kinds = _ddpg_path_run("default")
        assert len(ref) > 100 and sorted(kinds) == [False, False, True, True]
        got, kinds_got = _ddpg_path_run(path)
        assert kinds_got == kinds
        _assert_bitwise(ref, got, path)


def test_det_steps_alternate_walk_and_replay():
    """replayed, walked, replayed, walked steps on ONE runtime (runtime.STEP_PLAN flipped between steps) equal four replayed steps
    bit for bit: what the two ways share -- the patched items' cache of last values, the input sets' `prefetched` marks -- survives
    the change of mode"""
    from ga_ddpg_amd import runtime
    seen = []

    def flip(agent, i, batch):
        runtime.STEP_PLAN = i % 2 == 0
        if agent._rt is not None:
            seen.append(agent._rt._replays())
    with _mode():
        for cfg_name, kind in (("ddpg_td3_aux.yaml", "ddpg"), ("bc_dagger_aux.yaml", "bc")):
            ref = _ddpg_path_run("default")[0] if kind == "ddpg" else _run_steps(cfg_name, kind, PATH_B, "default", nsteps=PATH_STEPS)
            del seen[:]
            with _path("default"):                  # (restores STEP_PLAN)
                got = _run_steps(cfg_name, kind, PATH_B, "default", nsteps=PATH_STEPS, before_step=flip)
            assert seen == [False, True, False]
            _assert_bitwise(ref, got, kind + ": alternating walked and replayed steps")


def test_det_steps_across_discarded_step_lists():
    """three steps, the step lists thrown away twice (agent.clip_grad, part of _step_key(), set to another value -- a list is built
    under it and never run -- and back), three more steps: the per-pass plans and their items outlive the compiled lists that
    were destroyed, and Plan.patch goes on writing through those items.  Replayed in C, this equals the same sequence walked from
    Python (engine.USE_C_PLANS off: no compiled handles at all) bit for bit"""
    cleared = []

    def before(agent, i, batch):
        if i != 3:
            return
        rt, keep = agent._rt, agent.clip_grad
        old = rt._step_plans["key"]
        agent.clip_grad = 2.0 * keep
        rt._step_plan(rt._set, False)
        cleared.append(rt._step_plans["key"] != old)
        agent.clip_grad = keep
        cleared.append(rt._step_key() == old)          # (step 3 finds another key than the cache's: cleared a second time)
    with _mode():
        runs = {}
        for path in ("default", "plan_py"):
            del cleared[:]
            with _path(path):
                runs[path] = _run_steps("ddpg_td3_aux.yaml", "ddpg", PATH_B, "default", nsteps=6, before_step=before)
            assert cleared == [True, True]
        assert len(runs["default"]) > 100
        _assert_bitwise(runs["default"], runs["plan_py"], "step lists discarded between steps: replayed vs walked")


def test_det_ddpg_eval_mode_step_with_unfused_optimiser():
    """update_parameters(test=True) after set_fused_optim(False), a non-policy and a policy step at B = 32: num_batches_tracked of
    both encoders and every running statistic stay, and the log equals the fused eval-mode step's"""
    from oracle.detfill import fill_running_stats_
    from ga_ddpg_amd.synth_data import sample_valid_batch
    rng = np.random.default_rng(78)
    batch = sample_valid_batch(_memory("ddpg_td3_aux.yaml", 6), PATH_B, rng)
    noise = rng.random((PATH_B, 6)).astype(np.float32)
    with _mode():
        for start in (1, 2):
            logs = {}
            for fused in (True, False):
                agent, nets = tstep._filled_agent("ddpg_td3_aux.yaml", 91)
                for name, net in nets.items():
                    fill_running_stats_(net, name, 91)
                agent.update_step = start
                agent.runtime(PATH_B, batch["point_state_batch"].shape[2]).set_fused_optim(fused)
                before = {k: v.detach().cpu().clone() for k, v in agent.state_feature_extractor.state_dict().items()
                          if "running" in k or "num_batches" in k}
                assert sum("num_batches" in k for k in before) >= 2 and any("value_encoder" in k for k in before) and len(before) >= 60
                logs[fused] = {k: float(v) for k, v in agent.update_parameters(batch, agent.update_step, 0, test=True, noise_u=noise).items()}
                torch.cuda.synchronize()
                after = agent.state_feature_extractor.state_dict()
                for k, v in before.items():
                    assert torch.equal(after[k].cpu(), v), "eval-mode step (fused=%s) touched %s" % (fused, k)
            assert logs[True].keys() == logs[False].keys() and len(logs[True]) == 11
            for k in logs[True]:
                assert np.float64(logs[True][k]).tobytes() == np.float64(logs[False][k]).tobytes(), (start, k, logs[True][k], logs[False][k])


def _routed_families(nsteps=1):
    """kernel families the GEMM launches of one B = 256 step routed to (engine's timed walk records gad_last_kernel per launch)"""
    from ga_ddpg_amd import engine
    engine.timing_start(capacity=512)
    try:
        _run_steps("ddpg_td3_aux.yaml", "ddpg", 256, "default", nsteps=nsteps)
    finally:
        engine.timing_stop()
    return set(engine.timing_routes().values())


def test_torch_deterministic_flag_switches_the_mode():
    """torch.use_deterministic_algorithms(True) turns the mode on (two schedules agree bitwise, only the tile kernels run); once
    restored, a default step routes to the specialised kernel families again"""
    special = ("stream", "wide", "skinny", "split")
    prev = torch.are_deterministic_algorithms_enabled()
    hip.set_option("deterministic", 0)
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert hip.get_option("deterministic") == 1
        a = _run_steps("ddpg_td3_aux.yaml", "ddpg", 64, "default", nsteps=2)
        assert hip._lib_det[0] == 1
        b = _run_steps("ddpg_td3_aux.yaml", "ddpg", 64, "serial", nsteps=2)
        _assert_bitwise(a, b, "serial under torch's flag")
        det_fams = _routed_families()
    finally:
        torch.use_deterministic_algorithms(prev)
    assert det_fams and all(not any(w in f for w in special) for f in det_fams), det_fams
    assert hip.get_option("deterministic") == 0
    fams = _routed_families()
    assert hip._lib_det[0] == 0
    assert any(any(w in f for w in special) for f in fams), fams


def test_det_parity_with_reference_goldens(golden_dir):
    with _mode():
        tstep.test_ddpg_steps_vs_reference_golden(golden_dir)
        tstep.test_bc_steps_vs_reference_golden(golden_dir)
        tstep.test_ddpg_step_B256_vs_oracle()


@pytest.mark.parametrize("op", ["group", "gather"])
def test_det_facade_backward_with_collisions(op):
    """every index in {0, 1, 2}: thousands of additions land on three points; two calls give the same bits, within f32
    summation error of a float64 index_add_ on the host"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    B, C, N, M, S = 4, 64, 4096, 512, 64
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 3, (B, M, S) if op == "group" else (B, M), generator=g, dtype=torch.int32)
    feats = torch.randn(B, C, N, generator=g)
    gout = torch.randn((B, C, M, S) if op == "group" else (B, C, M), generator=g)
    fn = pu.grouping_operation if op == "group" else pu.gather_operation
    with _mode():
        outs = []
        for _ in range(2):
            f = feats.cuda().requires_grad_(True)
            fn(f, idx.cuda()).backward(gout.cuda())
            outs.append(f.grad.detach().cpu())
    assert torch.equal(outs[0], outs[1])
    ref = torch.zeros(B, C, N, dtype=torch.float64)
    flat_idx = idx.reshape(B, -1).long()
    for b in range(B):
        ref[b].index_add_(1, flat_idx[b], gout[b].reshape(C, -1).double())
    n_per = flat_idx.shape[1]
    tol = 2 * n_per * 6e-8 * gout.abs().max().item()
    assert (outs[0].double() - ref).abs().max().item() <= tol
    assert torch.count_nonzero(outs[0][:, :, 3:]) == 0
