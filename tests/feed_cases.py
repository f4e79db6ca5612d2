"""What the minibatch feeding tests share (tests/test_feed_matrix_host.py, tests/test_gpu_feed_matrix.py): the draws of a synchronous
loop, and a consumer that models what the fused runtime does with a minibatch -- and nothing else -- so that the feeding paths of
core.train_test_offline.train_off_policy can be held to those draws without a GPU."""
import threading
import time

import numpy as np

from ga_ddpg_amd.core.prefetch import KEYS


def _f32(v):
    return np.array(v.numpy() if hasattr(v, "numpy") else v, dtype=np.float32, copy=True)


def sync_draws(mem, B, n, seed):
    """the n minibatches a synchronous mem.sample(B, rng=default_rng(seed)) loop yields, as float32 copies"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        b = mem.sample(B, rng=rng)
        out.append({k: _f32(b[k]) for k in KEYS})
    return out


def all_draws_valid(mem, B, n, seed):
    """True when none of those n draws would be rejected by synth_data.sample_valid_batch (an expert, a positive-return and an
    unperturbed row in each): a sample_valid_batch loop on the same stream then yields exactly sync_draws()"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        idx = mem.draw_indices(B, rng)
        if not ((mem.expert_flags[idx] >= 1).any() and (mem.returns[idx] > 0).any() and (mem.perturb_flags[idx] < 1).any()):
            return False
    return True


def fill_time(mem, B):
    """seconds one synchronous draw + float32 copy takes on this memory: the median of five"""
    rng = np.random.default_rng(0)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        b = mem.sample(B, rng=rng)
        _ = {k: _f32(b[k]) for k in KEYS}
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


class _Joins(object):
    """stands where the runtime puts st["ev_up"]: synchronize() returns once the copy out of the staging buffers has run"""

    def __init__(self, thread):
        self._thread = thread

    def synchronize(self):
        self._thread.join()


class _PendingLog(dict):
    """update_parameters(sync=False)'s log: the first read waits for the step (core.agent.PendingLog)"""

    def __init__(self, thread, values):
        dict.__init__(self, values)
        self._thread = thread

    def items(self):
        self._thread.join()
        return dict.items(self)


class RecordingAgent(object):
    """Stands in for an agent inside train_off_policy.  update_parameters() keeps the runtime's contract with the producer of its
    minibatch: the batch is read some host time after it was handed over (`pause`: the lookahead draw, the enqueue), by an
    asynchronous copy that takes `pause` again (the worker thread: the host-to-device copies out of pinned memory); a batch that
    carries an "uploaded_event" entry gets there an object whose synchronize() returns when that copy is done
    (FusedRuntime._stage_inputs: st["ev_up"]).  `seen[i]` is what the copy of update i read."""

    def __init__(self, pause):
        self.pause = float(pause)
        self.update_step = 0
        self.seen = []
        self.hints = []
        self._workers = []

    def get_lr(self):
        return {"policy_lr": 0.0, "feature_lr": 0.0, "value_lr": 0.0}

    def step_scheduler(self, step=None):
        pass

    def prefetch(self, batch_data):
        self.hints.append(batch_data)
        return False

    def update_parameters(self, batch_data, updates, k, sync=True):
        time.sleep(self.pause)
        slot = len(self.seen)
        self.seen.append(None)

        def copy():
            time.sleep(self.pause)
            self.seen[slot] = {key: _f32(batch_data[key]) for key in KEYS}
        worker = threading.Thread(target=copy, name="feed-cases-copy", daemon=True)
        worker.start()
        self._workers.append(worker)
        if "uploaded_event" in batch_data:
            batch_data["uploaded_event"] = _Joins(worker)
        self.update_step += 1
        if sync:
            worker.join()
            return {"bc_loss": float(slot)}
        return _PendingLog(worker, {"bc_loss": float(slot)})

    def flush(self):
        for w in self._workers:
            w.join()


def corrupted(seen, want):
    """[(update, key)] where what the consumer's copy read is not the synchronous draw, bit for bit"""
    bad = []
    for i, (got, ref) in enumerate(zip(seen, want)):
        for k in KEYS:
            if got is None or got[k].shape != ref[k].shape or got[k].tobytes() != ref[k].tobytes():
                bad.append((i, k))
    return bad
