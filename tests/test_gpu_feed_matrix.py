"""Every minibatch feed x every loop of train_off_policy on the GPU, in deterministic mode, against bit equality: whatever overlaps
the sampling with the update -- a producer thread with pinned staging sets, the HBM mirror's lazy handles, the lookahead draw,
run-ahead -- the update steps must leave the bits of the plain synchronous loop over memory.sample on the same random stream.
B = 32, five updates per epoch, two epochs, a 1500-transition synthetic buffer.  (tests/test_feed_matrix_host.py holds the host
side of the same matrix against a consumer with controlled timing; here the timing is the hardware's.)"""
import contextlib
import functools
import os
import random

import numpy as np
import pytest
import torch

from tests import test_gpu_step as tstep
from tests.test_gpu_deterministic import _assert_bitwise, _mode, _state

pytestmark = pytest.mark.gpu
DDPG, BC = "ddpg_td3_aux.yaml", "bc_dagger_aux.yaml"
B, UPDATES, EPOCHS, DEPTH = 32, 5, 2, 2
N = UPDATES * EPOCHS
IDX_SEED = {DDPG: 4, BC: 4, "mixed": 4}        # every minibatch of these streams is valid (_assert_valid_draws)
LOOPS = ("plain", "lookahead", "run_ahead")


@contextlib.contextmanager
def _loop_env(loop):
    saved = os.environ.get("GAD_TRAIN_LOOKAHEAD")
    os.environ["GAD_TRAIN_LOOKAHEAD"] = "0" if loop == "plain" else "1"
    try:
        yield
    finally:
        if saved is None:
            del os.environ["GAD_TRAIN_LOOKAHEAD"]
        else:
            os.environ["GAD_TRAIN_LOOKAHEAD"] = saved


@functools.lru_cache(maxsize=None)
def _memory(cfg_name):
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    mem = BaseMemory(1500, load_cfg(cfg_name), point_dtype=np.float32)
    fill_synthetic_buffer(mem, 1500, seed=5)
    return mem


@functools.lru_cache(maxsize=None)
def _online_memory():
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    mem = BaseMemory(300, load_cfg(DDPG), name="online", point_dtype=np.float32)
    fill_synthetic_buffer(mem, 260, seed=32)
    return mem


def _valid(mems, idx):
    flags = [np.concatenate([np.asarray(getattr(m, name)[i]).reshape(-1) for m, i in zip(mems, idx)])
             for name in ("expert_flags", "returns", "perturb_flags")]
    return (flags[0] >= 1).any() and (flags[1] > 0).any() and (flags[2] < 1).any()


def _assert_valid_draws(mems, seed):
    """every minibatch of the stream has an expert, a positive-return and an unperturbed row (the masked means of the update are NaN
    otherwise): a property of the seeded buffers and the seed, read from the indices the way tests.test_gpu_bc_pipeline does"""
    rng = np.random.default_rng(seed)
    for i in range(N):
        idx = [m.draw_indices(B, rng) for m in mems]                  # list order: expert first, as sample_mixed draws
        assert _valid(mems, idx), "draw %d of index seed %d is not a valid minibatch" % (i, seed)


def _train(cfg_name, feed, loop, online=False):
    """one train_off_policy run -> (loss history as float64 arrays, _state, the agent's update_step).  Call inside _mode()."""
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    from ga_ddpg_amd.experiments.config import load_cfg
    mem = _memory(cfg_name)
    config = load_cfg(cfg_name).RL_TRAIN
    config.batch_size, config.updates_per_step, config.save_epoch = B, UPDATES, []
    assert config.max_epoch > 100
    seed = IDX_SEED["mixed" if online else cfg_name]
    _assert_valid_draws((mem, _online_memory()) if online else (mem,), seed)
    random.seed(91)
    np.random.seed(91)
    torch.manual_seed(91)                        # the TD3 noise comes from torch's device generator: the same draws in every run
    agent, nets = tstep._filled_agent(cfg_name, 17)
    rng = np.random.default_rng(seed)
    keeps = 2 if loop == "lookahead" else 1      # the lookahead loop holds two minibatches: a host sampler must keep two valid
    sampler, kw = None, {}
    if feed == "memory":
        kw = dict(sample=lambda batch_size: mem.sample(batch_size, rng=rng), device_replay=False)
    elif feed == "prefetch_copy":                # the producer thread copies the sampled clouds into the pinned set
        sampler = PrefetchSampler(mem, B, depth=DEPTH, outstanding=keeps, sample=lambda n: mem.sample(n, rng=rng))
        assert not sampler._direct
    elif feed == "prefetch_direct":              # the gather threads write the clouds into the pinned set
        sampler = PrefetchSampler(mem, B, depth=DEPTH, outstanding=keeps, rng=rng)
        assert sampler._direct and sampler._pool is not None
    elif feed == "mirror":
        kw = dict(device_replay=True, rng=rng)
    elif feed == "prefetch_mirror":
        sampler = PrefetchSampler(tto.device_mirror(mem), B, depth=DEPTH, rng=rng)
        assert sampler.lazy and sampler.max_outstanding is None
    elif feed == "mixed_mirror":
        kw = dict(device_replay=True, rng=rng)
    elif feed == "prefetch_mixed":
        assert config.onpolicy and int(B * config.online_buffer_ratio) == B
        sampler = PrefetchSampler(tto.mixed_device_mirror(mem, _online_memory(), B, B), 2 * B, depth=DEPTH, rng=rng)
        assert sampler.lazy and sampler.max_outstanding is None
    else:
        raise ValueError(feed)
    if sampler is not None:
        kw = dict(sample=sampler, device_replay=False)
    if online:
        kw["online_memory"] = _online_memory()
    hinted = []
    inner = agent.prefetch
    agent.prefetch = lambda b: hinted.append(inner(b)) or hinted[-1]
    try:
        with _loop_env(loop):
            losses, epochs = tto.train_off_policy(agent, mem, config, max_epochs=EPOCHS, run_ahead=(loop == "run_ahead"), **kw)
    finally:
        if sampler is not None:
            sampler.close()
    agent.flush()
    torch.cuda.synchronize()
    assert epochs == EPOCHS
    hist = {k: np.asarray(list(h), dtype=np.float64) for k, h in losses.items()}
    assert len(hist["bc_loss"]) == N + 1 and all(np.isfinite(h).all() for h in hist.values())       # deque([0]) + 10 updates
    assert np.unique(hist["bc_loss"][1:]).size == N                                                 # the minibatches do differ
    if loop == "lookahead":                      # the loop did draw ahead, and held two minibatches; the deterministic mode runs
        assert len(hinted) == N - 1 and not any(hinted)                # on one stream and takes no hint (the tests below do)
    else:
        assert not hinted
    if sampler is not None:
        assert len(sampler._sets) <= DEPTH + 2
        if not sampler.lazy:
            assert sampler.pin and len(sampler._sets) >= 2
            assert all(t.is_pinned() for st in sampler._sets for t in st.values())
    return hist, _state(agent, nets, []), agent.update_step


@functools.lru_cache(maxsize=None)
def _baseline(cfg_name):
    """the plain loop over memory.sample(rng=default_rng(seed)), host batches uploaded synchronously.  Call inside _mode()."""
    return _train(cfg_name, "memory", "plain")


def _assert_same_run(got, want, what):
    hist, state, step = got
    assert step == want[2]
    bad = [k for k in want[0] if hist[k].tobytes() != want[0][k].tobytes()]
    assert not bad, "%s: loss history differs in %s: %s vs %s" % (what, bad, hist[bad[0]], want[0][bad[0]])
    _assert_bitwise(want[1], state, what)


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("feed", ["prefetch_copy", "prefetch_direct", "mirror", "prefetch_mirror"])
def test_ddpg_feed_matrix_bitwise(feed, loop):
    with _mode():
        want = _baseline(DDPG)
        assert len(want[1]) > 100
        _assert_same_run(_train(DDPG, feed, loop), want, "DDPG %s / %s" % (feed, loop))


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("feed", ["prefetch_direct", "prefetch_mirror"])
def test_bc_feed_matrix_bitwise(feed, loop):
    with _mode():
        want = _baseline(BC)
        assert len(want[1]) > 100
        _assert_same_run(_train(BC, feed, loop), want, "BC %s / %s" % (feed, loop))


def test_memory_feed_under_lookahead_bitwise():
    """the control: fresh host arrays per draw, drawn ahead"""
    with _mode():
        for cfg_name in (DDPG, BC):
            _assert_same_run(_train(cfg_name, "memory", "lookahead"), _baseline(cfg_name), cfg_name + " memory.sample / lookahead")


def test_mixed_feed_behind_prefetch_sampler_bitwise():
    """expert + online minibatches (32 + 32 rows): MixedDeviceReplay handles prefetched by a PrefetchSampler and drawn ahead, against
    train_off_policy's own mixed mirror in the plain loop"""
    with _mode():
        want = _train(DDPG, "mixed_mirror", "plain", online=True)
        _assert_same_run(_train(DDPG, "prefetch_mixed", "lookahead", online=True), want, "mixed handles behind PrefetchSampler / lookahead")


# ------------------------------------------------------------------------------------------------ a hint that is not followed
def _zero_lr(agent):
    for name in ("policy_optim", "critic_optim", "state_feat_encoder_optim", "state_feat_val_encoder_optim"):
        for g in getattr(getattr(agent, name, None), "param_groups", []):
            g["lr"] = 0.0


def _hinted_steps(cfg_name, hint, taken, zero_lr):
    """six steps over lazy handles of the mirror; with `hint`, agent.prefetch() goes in front of steps 1 and 2 with handles that no
    step ever gets, in front of step 3 (for DDPG a walked eval-mode step, which drops it) with step 4's handle and in front of step 4
    with step 5's.  taken: what prefetch() must return once the runtime exists.  Every step's input buffers are compared with
    memory.sample on its indices.  -> (_state, [the logs])"""
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    from ga_ddpg_amd.runtime import BATCH_KEYS
    from tests.test_gpu_bc_pipeline import _valid_indices
    mem = _memory(cfg_name)
    idx = _valid_indices(mem, B, 8, 21)
    ddpg = cfg_name == DDPG
    random.seed(91)
    np.random.seed(91)
    torch.manual_seed(91)
    dmem = DeviceReplay(mem)
    agent, nets = tstep._filled_agent(cfg_name, 23)
    if zero_lr:
        _zero_lr(agent)
    results, inputs = [], []

    def step(i, handle=None, **kw):
        handle = dmem.sample_lazy(B, batch_idx=idx[i]) if handle is None else handle
        results.append(agent.update_parameters(handle, agent.update_step, i, **kw))
        agent.step_scheduler(agent.update_step)
        torch.cuda.synchronize()
        inputs.append({k: agent._rt.dbuf[k].detach().cpu().clone() for k in BATCH_KEYS})
    first = dmem.sample_lazy(B, batch_idx=idx[0])
    assert agent.prefetch(first) is False                                # no runtime before the first step
    step(0, handle=first)
    for i in (1, 2):                                                     # staged behind step i, and step i + 1 gets another minibatch
        if hint:
            assert agent.prefetch(dmem.sample_lazy(B, batch_idx=idx[5 + i])) is taken
        step(i)
    h4 = dmem.sample_lazy(B, batch_idx=idx[4])
    if hint:
        assert agent.prefetch(h4) is taken
    step(3, **({"test": True} if ddpg else {}))                          # DDPG: walked, the hint in front of it is never staged
    h5 = dmem.sample_lazy(B, batch_idx=idx[5])                           # the ring of index staging sets still hands one out
    if hint:
        assert agent.prefetch(h5) is taken
    step(4, handle=h4)
    step(5, handle=h5)                                                   # ... and a hint that IS followed
    agent.flush()
    results = [{k: float(v) for k, v in r.items()} for r in results]
    assert all(np.isfinite(list(r.values())).all() for r in results)
    want_inputs = [mem.sample(B, batch_idx=idx[i]) for i in range(6)]
    for i, (got, ref) in enumerate(zip(inputs, want_inputs)):           # every step read ITS minibatch, whatever was hinted
        for k in BATCH_KEYS:
            if k == "next_point_state_batch" and not ddpg:             # (a BC step reads no next-state cloud: never filled)
                continue
            np.testing.assert_array_equal(got[k].numpy(), np.asarray(ref[k], dtype=np.float32).reshape(got[k].shape),
                                          err_msg="step %d %s" % (i, k))
    return _state(agent, nets, results), results


@pytest.mark.parametrize("cfg_name", [DDPG, BC])
def test_dropped_prefetch_hint_bitwise_in_deterministic_mode(cfg_name):
    """the deterministic mode runs on one stream and takes no hint (prefetch() -> False): hinted or not, the same bits"""
    with _mode():
        want, _ = _hinted_steps(cfg_name, False, False, False)
        assert len(want) > 100
        got, _ = _hinted_steps(cfg_name, True, False, False)
        _assert_bitwise(want, got, cfg_name + ": hints in deterministic mode")


@pytest.mark.parametrize("cfg_name", [DDPG, BC])
def test_dropped_prefetch_hint_is_dropped(cfg_name):
    """default mode: prefetch(X) -> True says the hint was TAKEN (staged behind the running step into the other input set), not that
    it will be used -- the next step may get another minibatch, or be walked.  A step that gets Y after prefetch(X) reads Y: its
    input buffers equal memory.sample on Y's indices bit for bit (_hinted_steps), and at learning rate 0, where a step's numbers
    depend on its minibatch only, its log equals the unhinted step's within the run-to-run noise of the float atomics
    (2e-4 relative, the bound tests/test_gpu_bc_pipeline.py and tests/test_gpu_api.py hold run-ahead steps to)."""
    from tests.helpers import assert_close
    _, want = _hinted_steps(cfg_name, False, True, True)
    _, got = _hinted_steps(cfg_name, True, True, True)
    assert abs(want[1]["bc_loss"] - want[2]["bc_loss"]) > 1e-4            # the minibatches do differ
    for s, (a, b) in enumerate(zip(want, got)):
        assert a.keys() == b.keys()
        for k in a:
            assert_close(b[k], a[k], 2e-4, 1e-6, "%s step %d %s" % (cfg_name, s, k))


