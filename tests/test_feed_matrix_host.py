"""Every host feeding path x every loop of train_off_policy, without a GPU: the update step must see the minibatches a synchronous
memory.sample loop on the same random stream draws, bit for bit and in order.  The consumer is tests.feed_cases.RecordingAgent,
which reads a minibatch the way the fused runtime does: late, and from another thread.

Feeds: "prefetch" = PrefetchSampler(mem, B, rng=...) over memory.sample (which takes clouds_out: the clouds land in the staging set
on four gather threads); "prefetch_direct" = the same through sample_valid_batch with two threads; "prefetch_callable" = a callable
without clouds_out, whose clouds the producer thread copies into the set; "memory" = memory.sample itself, the control.

The pause between "handed over" and "read" is a stimulus, not a tolerance: ten times what one draw + copy takes on this buffer (at
least 0.05 s), so that a producer that is allowed to refill a staging set too early always gets there first."""
import functools
import threading
import time

import numpy as np
import pytest

from tests import feed_cases as fc
from tests.test_prefetch import _memory

B, UPDATES, EPOCHS, SEED = 16, 8, 2, 11
N = UPDATES * EPOCHS
LIMIT = 60.0
ALIVE = {"plain": 1, "lookahead": 2, "run_ahead": 1}       # minibatches the loop holds at once (run-ahead: guarded by the events)


@functools.lru_cache(maxsize=None)
def _case_data():
    mem = _memory()
    fill = fc.fill_time(mem, B)
    pause = max(10.0 * fill, 0.05)
    print("feed matrix: one draw + copy takes %.6f s, pause %.3f s" % (fill, pause))
    # every draw of this stream passes sample_valid_batch's test: the callables that reject draws yield mem.sample's batches
    assert fc.all_draws_valid(mem, B, N, SEED)
    return mem, fc.sync_draws(mem, B, N, SEED), pause


def _config():
    from ga_ddpg_amd.experiments.config import load_cfg
    config = load_cfg("ddpg_td3_aux.yaml").RL_TRAIN
    config.batch_size, config.updates_per_step = B, UPDATES
    assert config.max_epoch > 10 * N
    return config


def _feed(kind, mem, depth, outstanding=None):
    """-> (sample= argument, the PrefetchSampler behind it or None)"""
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    from ga_ddpg_amd.synth_data import sample_valid_batch
    rng = np.random.default_rng(SEED)
    kw = {} if outstanding is None else {"outstanding": outstanding}
    if kind == "memory":
        return (lambda batch_size: mem.sample(batch_size, rng=rng)), None
    if kind == "prefetch":
        s = PrefetchSampler(mem, B, depth=depth, rng=rng, pin=False, **kw)         # memory.sample: takes clouds_out, four gather threads
    elif kind == "prefetch_direct":
        s = PrefetchSampler(mem, B, depth=depth, pin=False, threads=2, **kw,
                            sample=lambda n, clouds_out=None, pool=None: sample_valid_batch(mem, n, rng, clouds_out, pool))
        assert s._direct and s._pool is not None
    else:
        s = PrefetchSampler(mem, B, depth=depth, pin=False, sample=lambda n: sample_valid_batch(mem, n, rng), **kw)
        assert not s._direct
    return s, s


def _in_thread(fn):
    """run fn on a thread joined with a limit: a deadlock (a free pool that never refills) is a failure, not a hang"""
    box = {}

    def body():
        try:
            box["value"] = fn()
        except BaseException as e:                      # noqa: B902 (handed to the test's thread)
            box["error"] = e
    t = threading.Thread(target=body, name="feed-matrix-case", daemon=True)
    t.start()
    t.join(LIMIT)
    assert not t.is_alive(), "the case did not finish within %.0f s: deadlock" % LIMIT
    if "error" in box:
        raise box["error"]
    return box["value"]


def _run_case(monkeypatch, feed, loop, depth, outstanding=None):
    from ga_ddpg_amd.core import train_test_offline as tto
    mem, want, pause = _case_data()
    monkeypatch.setenv("GAD_TRAIN_LOOKAHEAD", "0" if loop == "plain" else "1")

    def case():
        sample, sampler = _feed(feed, mem, depth, outstanding)
        agent = fc.RecordingAgent(pause)
        try:
            losses, epochs = tto.train_off_policy(agent, mem, _config(), max_epochs=EPOCHS, sample=sample,
                                                  run_ahead=(loop == "run_ahead"), device_replay=False)
        finally:
            took = 0.0
            if sampler is not None:                     # the consumer still holds its last batch(es): close() must not wait for them
                t0 = time.perf_counter()
                sampler.close()
                took = time.perf_counter() - t0
        agent.flush()
        return agent, sampler, losses, epochs, took
    agent, sampler, losses, epochs, took = _in_thread(case)
    assert epochs == EPOCHS and agent.update_step == N and len(agent.seen) == N
    assert [float(v) for v in list(losses["bc_loss"])[-N:]] == [float(i) for i in range(N)]        # every log, in order
    bad = fc.corrupted(agent.seen, want)
    torn = sorted({i for i, _ in bad})
    assert not bad, "%s / %s / depth %d: %d of %d minibatches differ from the synchronous draws (updates %s), e.g. %s" % (
        feed, loop, depth, len(torn), N, torn, bad[:4])
    if sampler is not None:
        assert took < 5.0, "close() took %.2f s" % took
        assert not sampler._thread.is_alive()
        assert len(sampler._sets) <= depth + ALIVE[loop], (len(sampler._sets), depth, loop)
    return agent, sampler


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("loop", ["plain", "lookahead", "run_ahead"])
@pytest.mark.parametrize("feed", ["prefetch", "prefetch_direct", "prefetch_callable", "memory"])
def test_feed_matrix_host(monkeypatch, feed, loop, depth):
    agent, sampler = _run_case(monkeypatch, feed, loop, depth)
    if loop == "lookahead" and feed == "memory":
        assert len(agent.hints) == N - 1                # the control does draw ahead: every minibatch but the first was hinted
    if loop != "lookahead":
        assert not agent.hints


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("feed", ["prefetch", "prefetch_direct"])
def test_two_outstanding_batches_under_lookahead(monkeypatch, feed, depth):
    """a sampler that keeps its two most recent minibatches valid is drawn ahead from: the loop holds two, and both stay whole"""
    agent, sampler = _run_case(monkeypatch, feed, "lookahead", depth, outstanding=2)
    assert sampler.max_outstanding == 2
    assert len(agent.hints) == N - 1


def test_one_outstanding_batch_runs_the_plain_loop(monkeypatch):
    """the default sampler keeps one minibatch valid: train_off_policy does not draw ahead from it, and says so once"""
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    mem, want, pause = _case_data()
    monkeypatch.setenv("GAD_TRAIN_LOOKAHEAD", "1")
    lines = []
    agent = fc.RecordingAgent(0.0)
    with PrefetchSampler(mem, B, rng=np.random.default_rng(SEED), pin=False) as s:
        assert s.max_outstanding == 1
        _in_thread(lambda: tto.train_off_policy(agent, mem, _config(), max_epochs=1, sample=s, device_replay=False, log=lines.append))
    assert not agent.hints and len(agent.seen) == UPDATES
    assert len([ln for ln in lines if "max_outstanding" in ln]) == 1, lines
    assert not fc.corrupted(agent.seen, want[:UPDATES])


@pytest.mark.parametrize("outstanding", [1, 2])
def test_producer_error_on_the_lookahead_draw(monkeypatch, outstanding):
    """the second draw -- the one the lookahead loop makes before the first update -- fails on the producer thread: the loop ends
    with the sampler's RuntimeError, not with a hang or a stale batch"""
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    mem, want, pause = _case_data()
    monkeypatch.setenv("GAD_TRAIN_LOOKAHEAD", "1")
    rng = np.random.default_rng(SEED)
    calls = []

    def sample(n):
        calls.append(n)
        if len(calls) == 2:
            raise ValueError("empty buffer")
        return mem.sample(n, rng=rng)
    agent = fc.RecordingAgent(0.0)
    s = PrefetchSampler(mem, B, depth=2, pin=False, sample=sample, outstanding=outstanding)

    def case():
        with pytest.raises(RuntimeError, match="prefetch thread failed") as err:
            tto.train_off_policy(agent, mem, _config(), max_epochs=EPOCHS, sample=s, device_replay=False)
        return err
    try:
        err = _in_thread(case)
    finally:
        s.close()
    assert isinstance(err.value.__cause__, ValueError)
    agent.flush()
    assert len(agent.seen) == (0 if outstanding == 2 else 1)       # drawn ahead: before the first update; else before the second
    assert not fc.corrupted(agent.seen, want[:len(agent.seen)])
