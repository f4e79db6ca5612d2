"""GPU-resident mirror of the replay buffer ("the step before the path").

The reference samples a minibatch on the host (core/replay_memory.py:166-176: fancy-index every array, two
(B,4,1030) float64 gathers = 17 MB per step) and ships 22 arrays to the device (core/agent.py:211-240).  At > 200
update steps/s that costs more than the update itself.  `DeviceReplay` keeps the arrays the update step reads in
HBM as float32 and performs the gather there; the INDEX arithmetic stays on the host and is the reference's,
so a minibatch drawn here equals `BaseMemory.sample` with the same `batch_idx` (tests/test_gpu_modules.py:
test_device_replay_matches_host_sampling).

    mem  = BaseMemory(...); mem.load(...) / filled by the environment loop
    dmem = DeviceReplay(mem)                     # one upload (cap x 4 x 1030 float32 for the clouds)
    batch = dmem.sample(256, rng)                # dict of CUDA tensors + host-side mask counts
    agent.update_parameters(batch, agent.update_step, k)

`refresh(lo, hi)` re-uploads a slice after the host buffer was written to (online training).

Hindsight relabelling (`memory.self_supervision` on a non-expert buffer, reference core/replay_memory.py:233-249,271-272) is
4x4 pose algebra on B rows, in one of two modes chosen per mirror:
  relabel="host" (default): the goals are formed by the SAME BaseMemory.onpolicy_goals the host path uses -- a Python loop with
    an eigen-decomposition per row, at handle-draw time -- and travel with the index vectors as a (B, 8) block
    [goal (7) | relabel flag]; the gather's goal rows are overwritten where the flag is set, so both paths train on
    bit-identical goals.
  relabel="device": the mirror also keeps `state_pose` (cap x 16 float32, 64 B a transition) and one gad_replay_relabel_goals
    launch behind the gather forms the goals of the on-policy rows from it by a float32 closed form (include/gaddpg.h
    section F); the host does no pose algebra.  Promise: rigid poses; goals equal the host's to float32 rounding, not bit for
    bit (tests/test_gpu_device_relabel.py); expert rows and every other key stay bit-identical.
A handle remembers the mode it was drawn in ("relabel_mode").
"""
import numpy as np
import torch

from .. import hip
from .replay_memory import written_slots

_ROW_KEYS = (("action", "action_batch"), ("expert_action", "expert_action_batch"), ("reward", "reward_batch"),
             ("returns", "return_batch"), ("terminal", "mask_batch"), ("goal", "goal_batch"),
             ("expert_flags", "expert_flag_batch"), ("perturb_flags", "perturb_flag_batch"))


class _Shape(object):
    """placeholder that only answers `.shape` (the agent sizes its runtime from point_state_batch.shape)"""

    def __init__(self, shape):
        self.shape = tuple(shape)


def _write_stamp(memory):
    """BaseMemory.write_stamp(), also for a buffer object that predates it"""
    if hasattr(memory, "write_stamp"):
        return memory.write_stamp()
    return (int(getattr(memory, "write_epoch", 0)), int(memory.cur_idx), int(memory.total_env_step), bool(memory.is_full))


_RING = 8       # index staging sets (a set is reused only after the gather that read it has run: `used` event)


def _take_stage_set(stage, n, device, ring=_RING):
    """the next handle's staging set out of `stage` (the owner's dict of rings, one per batch size): dict(host = pinned (3,n)
    int64, dev = device (3,n) int64, copied = event of the host -> device copy, used = event recorded after the LAST gather that read `dev`, or None).  The copies run on a
    stream of their own and the handle carries `copied`: a runtime that enqueues steps ahead of the GPU
    (update_parameters(sync=False)) starts the gather as soon as the indices are on the device, not after everything
    queued on the caller's stream.  Reuse is guarded by BOTH events: the pinned block by the copy that read it, the
    device block by the gather that read it -- however far ahead handles are drawn (PrefetchSampler depth, host ring),
    a set never changes under a gather that is still queued; a set whose handle has not been gathered at all yet
    (`pending`) is skipped, and the ring grows if every set is held that way.  Shared by DeviceReplay and
    MixedDeviceReplay."""
    key = ("sets", n)
    sets = stage.get(key)
    if sets is None:
        sets = stage[key] = {"next": 0, "items": [None] * ring}
    items = sets["items"]
    j = sets["next"]
    for _ in range(len(items)):              # a set whose handle has not been gathered yet is never handed out again
        if items[j] is None or not items[j]["pending"]:
            break
        j = (j + 1) % len(items)
    else:                                    # every set is held by a handle drawn ahead of its use: grow the ring
        if len(items) >= 64:
            raise RuntimeError("DeviceReplay: 64 sample_lazy() handles are outstanding (drawn but never passed to an "
                               "update step); drop-and-redraw loops should use sample() instead")
        items.append(None)
        j = len(items) - 1
    sets["next"] = (j + 1) % len(items)
    it = items[j]
    if it is None:
        it = items[j] = {"host": torch.empty(3, n, dtype=torch.int64).pin_memory(),
                         "dev": torch.empty(3, n, dtype=torch.int64, device=device),
                         "ghost": torch.zeros(n, 8, dtype=torch.float32).pin_memory(),       # [relabelled goal | flag]
                         "gdev": torch.zeros(n, 8, dtype=torch.float32, device=device),
                         "copied": torch.cuda.Event(), "used": None, "pending": False}
    else:
        it["copied"].synchronize()           # the copy that last read this pinned block
        if it["used"] is not None:
            it["used"].synchronize()         # the gather(s) that read the device block
    it["pending"] = True
    return it


def _upload_stage_set(it, copy_stream, refresh_events, relabel):
    """host -> device copy of a filled staging set on `copy_stream`, after every upload of buffer content the handle's gather
    will read (`refresh_events`); records the set's `copied` event"""
    for ev in refresh_events:
        if ev is not None:
            copy_stream.wait_event(ev)
    with torch.cuda.stream(copy_stream):
        it["dev"].copy_(it["host"], non_blocking=True)
        if relabel:
            it["gdev"].copy_(it["ghost"], non_blocking=True)
        it["copied"].record(copy_stream)
    it["relabel"] = relabel


def _launch_relabel(B, row_start, srcs, idx, end, goal):
    """one gad_replay_relabel_goals launch on the current stream, behind the gather / index_select that wrote `goal` (B, 7):
    srcs[s] = (state_pose, expert_flags) of a source whose on-policy rows get hindsight goals, or None"""
    a = hip.ReplayRelabelArgs()
    a.B, a.n_src = int(B), len(srcs)
    for s, r in enumerate(row_start):
        a.row_start[s] = int(r)
    for s, src in enumerate(srcs):
        if src is not None:
            a.src[s].state_pose, a.src[s].expert_flags = hip.ptr(src[0]), hip.ptr(src[1])
    a.idx, a.end, a.out_goal = hip.ptr(idx), hip.ptr(end), hip.ptr(goal)
    hip.call_struct("gad_replay_relabel_goals", a)


def _stage_set_used(it, stream):
    """the staging set is not rewritten before what was just enqueued on `stream` has read it"""
    if it["used"] is None:
        it["used"] = torch.cuda.Event()
    it["used"].record(stream)
    it["pending"] = False


class DeviceReplay(object):
    def __init__(self, memory, device=None, relabel="host"):
        if relabel not in ("host", "device"):
            raise ValueError("DeviceReplay: relabel must be \"host\" or \"device\", got %r" % (relabel,))
        self.memory = memory
        self.relabel = relabel
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceReplay needs a GPU (the update path has no CPU fallback)")
        cap = memory.point_state.shape[0]
        self.cap = cap
        f32 = dict(dtype=torch.float32, device=self.device)
        self.point_state = torch.empty(tuple(memory.point_state.shape), **f32)
        self.rows = {src: torch.empty(tuple(getattr(memory, src).shape), **f32) for src, _ in _ROW_KEYS}
        self.timestep = torch.empty(cap, **f32)
        # relabel="device" only: the poses the hindsight goals are formed from (64 B a transition)
        self.state_pose = torch.empty(cap, 16, **f32) if relabel == "device" else None
        self._stage = {}
        self._copy_stream = None
        self._ev_refresh = None
        self.uploaded_cloud_rows = 0             # running count of cloud rows sent to the device (refresh + sync_writes)
        self.refresh()
        self._stamp = _write_stamp(memory)

    # ------------------------------------------------------------------ host -> device
    def refresh(self, lo=0, hi=None):
        """(re-)upload transitions [lo, hi) of the host buffer"""
        m = self.memory
        hi = self.cap if hi is None else hi
        if hi <= lo:
            return
        sl = slice(lo, hi)
        # float64 -> float32 on the host in bounded chunks (the cloud array is 33 KB per transition)
        self._upload_clouds(lo, hi)
        self._upload_rows(sl)
        self._refreshed()

    def _upload_clouds(self, lo, hi, step=4096):
        m = self.memory
        for a in range(lo, hi, step):
            b = min(a + step, hi)
            self.point_state[a:b].copy_(torch.from_numpy(np.ascontiguousarray(m.point_state[a:b], dtype=np.float32)))
        self.uploaded_cloud_rows += hi - lo

    def _upload_rows(self, sl):
        m = self.memory
        for src, _ in _ROW_KEYS:
            self.rows[src][sl].copy_(torch.from_numpy(np.ascontiguousarray(getattr(m, src)[sl], dtype=np.float32)))
        self.timestep[sl].copy_(torch.from_numpy(np.ascontiguousarray(m.timestep[sl], dtype=np.float32)))
        if self.state_pose is not None:
            self.state_pose[sl].copy_(torch.from_numpy(np.ascontiguousarray(m.state_pose[sl], dtype=np.float32).reshape(-1, 16)))

    def _refreshed(self):
        if self._ev_refresh is None:
            self._ev_refresh = torch.cuda.Event()
        self._ev_refresh.record(torch.cuda.current_stream())      # later handles become ready after this upload

    def sync_writes(self):
        """bring the mirror up to date after the host buffer was written (online training: rollouts land between epochs).
        Clouds -- 16.5 KB a transition, all but 0.6 % of the bytes -- go up for exactly the slots push() wrote since the last
        sync (replay_memory.written_slots, from the cursor stamps), as runs of neighbouring slots; the small row arrays
        (104 B a transition, 168 B with the poses of relabel="device") go up whole over [0, upper_idx()), which also carries
        add_episode's back-filled returns of earlier slots.  Stamps that pushes alone do not explain (reset, load, direct writes announced by mark_rewritten(),
        more pushes than the buffer holds) -> refresh(0, upper_idx()).  -> number of cloud rows uploaded."""
        m = self.memory
        stamp = _write_stamp(m)
        if stamp == self._stamp:
            return 0
        before = self.uploaded_cloud_rows
        slots = written_slots(self._stamp, stamp, self.cap, int(getattr(m, "buffer_start_idx", 0)))
        hi = m.upper_idx()
        if slots is None:
            self.refresh(0, hi)
        else:
            if len(slots):
                cuts = np.flatnonzero(np.diff(slots) != 1) + 1          # runs of neighbouring slots: one copy each
                for run in np.split(slots, cuts):
                    self._upload_clouds(int(run[0]), int(run[-1]) + 1)
            self._upload_rows(slice(0, hi))
            self._refreshed()
        self._stamp = stamp
        return self.uploaded_cloud_rows - before

    RING = _RING

    def _stage_set(self, n):
        return _take_stage_set(self._stage, n, self.device, self.RING)

    def _relabels(self):
        m = self.memory
        return bool(getattr(m, "self_supervision", False)) and getattr(m, "name", "") != "expert"

    def _indices3(self, idx, nxt, end):
        it = self._stage_set(idx.shape[0])
        host, dev, ev = it["host"], it["dev"], it["copied"]
        h = host.numpy()
        h[0], h[1], h[2] = idx, nxt, end
        relabel = self._relabels()
        it["relabel_device"] = relabel and self.relabel == "device"      # formed behind the gather, from the mirrored poses
        relabel = relabel and self.relabel == "host"
        if relabel:                              # hindsight goals of the on-policy rows (BaseMemory.post_process_batch)
            mask, goal, _ = self.memory.onpolicy_goals(idx)
            g = it["ghost"].numpy()
            g[:, :7] = goal
            g[:, 7] = np.asarray(mask, dtype=np.float32).reshape(-1)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        _upload_stage_set(it, self._copy_stream, (self._ev_refresh,), relabel)
        return dev, ev, it

    @staticmethod
    def _apply_relabel(it, goal):
        """goal rows <- the staged hindsight goals where their flag is set (same stream as the gather that wrote `goal`)"""
        g = it["gdev"]
        goal.copy_(torch.where(g[:, 7:8] > 0, g[:, :7], goal))

    def _relabel_on_device(self, it, goal):
        """goal rows of the on-policy rows <- hindsight goals formed from the mirrored poses (same stream as the gather that wrote
        `goal`, whose index vectors the launch reads: call it before _stage_set_used)"""
        dev = it["dev"]
        _launch_relabel(dev.shape[1], (0, dev.shape[1]), [(self.state_pose, self.rows["expert_flags"])], dev[0], dev[2], goal)

    # ------------------------------------------------------------------ sampling
    def sample_lazy(self, batch_size, rng=None, batch_idx=None):
        """like sample(), but nothing is gathered yet: the returned dict carries the device index vectors and
        `FusedRuntime.upload` fills its static input buffers with ONE gad_replay_gather launch (no intermediate
        tensors, no device-to-device copies).  `point_state_batch` is a shape-only placeholder."""
        m = self.memory
        if batch_idx is None:
            batch_idx = m.draw_indices(batch_size, rng)
        batch_idx = np.asarray(batch_idx, dtype=np.int64)
        nxt = m.next_indices(batch_idx)
        end = np.asarray(m.episode_map[batch_idx], dtype=np.int64)
        B = batch_idx.shape[0]
        dev, ev, it = self._indices3(batch_idx, nxt, end)
        return {"replay_gather": self, "idx": dev[0], "nxt": dev[1], "end": dev[2], "ready_event": ev, "_stage_set": it,
                "relabel_mode": self.relabel, "batch_idx": np.uint8(batch_idx),
                "point_state_batch": _Shape((B,) + tuple(self.point_state.shape[1:])),
                "mask_counts": self._mask_counts(batch_idx)}

    def gather_into(self, lazy, dbuf):
        """fill the runtime's static batch buffers (dict of CUDA float32 tensors) from a sample_lazy() handle.  Ordered on
        the CURRENT stream after the handle's index upload (which ran on the copy stream), whoever the caller is."""
        cur = torch.cuda.current_stream()
        if lazy.get("ready_event") is not None:
            cur.wait_event(lazy["ready_event"])
        a = hip.ReplayGatherArgs()
        a.B = int(lazy["idx"].shape[0])
        a.cloud_elems = int(self.point_state.shape[1] * self.point_state.shape[2])
        a.idx, a.nxt, a.end = hip.ptr(lazy["idx"]), hip.ptr(lazy["nxt"]), hip.ptr(lazy["end"])
        a.point_state = hip.ptr(self.point_state)
        for src in ("action", "expert_action", "goal", "reward", "returns", "terminal", "expert_flags", "perturb_flags"):
            setattr(a, src, hip.ptr(self.rows[src]))
        a.timestep = hip.ptr(self.timestep)
        a.out_point, a.out_next_point = hip.ptr(dbuf["point_state_batch"]), hip.ptr(dbuf["next_point_state_batch"])
        for dst, key in (("out_action", "action_batch"), ("out_expert_action", "expert_action_batch"), ("out_goal", "goal_batch"),
                         ("out_reward", "reward_batch"), ("out_return", "return_batch"), ("out_mask", "mask_batch"),
                         ("out_time", "time_batch"), ("out_time_m1", "time_m1"), ("out_expert_flag", "expert_flag_batch"),
                         ("out_perturb_flag", "perturb_flag_batch")):
            setattr(a, dst, hip.ptr(dbuf[key]))
        hip.call_struct("gad_replay_gather", a)
        it = lazy.get("_stage_set")
        if it is not None and it.get("relabel"):
            self._apply_relabel(it, dbuf["goal_batch"])
        if it is not None and it.get("relabel_device"):
            self._relabel_on_device(it, dbuf["goal_batch"])
        if it is not None:                       # the staging set is not rewritten before this gather has run
            _stage_set_used(it, cur)

    def release(self, lazy):
        """give back the staging set of a sample_lazy() handle that will never be passed to an update step (a prefetcher
        closing with handles in flight, a batch dropped by a validity check): without this the set stays `pending` and
        is never handed out again"""
        it = lazy.get("_stage_set") if isinstance(lazy, dict) else None
        if it is not None:
            it["pending"] = False

    def _mask_counts(self, batch_idx):
        m = self.memory
        ret = np.asarray(m.returns[batch_idx]).reshape(-1)
        exp = np.asarray(m.expert_flags[batch_idx]).reshape(-1)
        per = np.asarray(m.perturb_flags[batch_idx]).reshape(-1)
        reward, expert = ret > 0, exp >= 1
        return np.array([(per < 1).sum(), reward.sum(), expert.sum(), (~(reward & expert)).sum()], dtype=np.float64)

    def sample(self, batch_size, rng=None, batch_idx=None):
        """the update step's 11 arrays as CUDA float32 tensors (runtime.BATCH_KEYS layout) + `batch_idx` and the
        host-side `mask_counts` the data-parallel path all-reduces.  Index semantics: BaseMemory.draw_indices /
        next_indices / post_process_batch (reference core/replay_memory.py:166-176,251-272)."""
        m = self.memory
        if batch_idx is None:
            batch_idx = m.draw_indices(batch_size, rng)
        batch_idx = np.asarray(batch_idx, dtype=np.int64)
        nxt = m.next_indices(batch_idx)
        end = np.asarray(m.episode_map[batch_idx], dtype=np.int64)
        dev, ev, it = self._indices3(batch_idx, nxt, end)
        cur = torch.cuda.current_stream()
        cur.wait_event(ev)
        d_idx, d_nxt, d_end = dev[0], dev[1], dev[2]
        out = {"point_state_batch": self.point_state.index_select(0, d_idx),
               "next_point_state_batch": self.point_state.index_select(0, d_nxt)}
        for src, dst in _ROW_KEYS:
            out[dst] = self.rows[src].index_select(0, d_idx)
        # remaining steps to the end of the episode (post_process_batch)
        out["time_batch"] = self.timestep.index_select(0, d_end) + 1.0 - self.timestep.index_select(0, d_idx)
        if it.get("relabel"):
            self._apply_relabel(it, out["goal_batch"])
        if it.get("relabel_device"):
            self._relabel_on_device(it, out["goal_batch"])
        _stage_set_used(it, cur)                 # the index_selects above read the staging set's device block
        out["batch_idx"] = np.uint8(batch_idx)
        out["mask_counts"] = self._mask_counts(batch_idx)
        return out


class MixedDeviceReplay(object):
    """One minibatch from several GPU-resident buffers: MixedDeviceReplay([(dmem_expert, n0), (dmem_online, n1), ...]) draws n_i
    rows from the i-th DeviceReplay and hands them to the update step as ONE batch of B = sum(n_i) rows, the first part's rows
    first -- the reference learner's expert + online minibatch (core/trainer.py:212-232; host form:
    replay_memory.sample_mixed).  Up to hip.REPLAY_MAX_SRC parts; a part of 0 rows is allowed.  Index arithmetic is each
    memory's own draw_indices / next_indices / episode_map, drawn in list order from one `rng`, so a minibatch equals
    sample_mixed with the same per-part indices.  Hindsight goals are formed for the rows of the parts whose memory relabels
    (DeviceReplay._relabels) only, in each part's own mode (DeviceReplay(relabel=...)): relabel="host" parts fill the staged (B, 8)
    block the gather applies, relabel="device" parts get ONE gad_replay_relabel_goals launch behind the gather (none when no such
    part relabels).  One gad_replay_gather_multi launch fills the step's input buffers (or sample()'s
    tensors); the handle of sample_lazy() follows DeviceReplay's contract, so FusedRuntime.upload / prefetch_inputs,
    PrefetchSampler and train_off_policy's lookahead take it as they take a DeviceReplay's."""

    RING = _RING

    def __init__(self, parts):
        parts = [(d, int(n)) for d, n in parts]
        if not 1 <= len(parts) <= hip.REPLAY_MAX_SRC:
            raise ValueError("MixedDeviceReplay takes 1..%d parts, got %d" % (hip.REPLAY_MAX_SRC, len(parts)))
        if any(n < 0 for _, n in parts) or sum(n for _, n in parts) < 1:
            raise ValueError("MixedDeviceReplay: the part sizes must be >= 0 and sum to at least 1")
        shapes = [tuple(d.point_state.shape[1:]) for d, _ in parts]
        if any(sh != shapes[0] for sh in shapes):
            raise ValueError("MixedDeviceReplay: the buffers store clouds of different shapes: %s" % (shapes,))
        if any(d.device != parts[0][0].device for d, _ in parts):
            raise ValueError("MixedDeviceReplay: the mirrors live on different devices")
        self.parts = [d for d, _ in parts]
        self.sizes = [n for _, n in parts]
        self.row_start = [0] + [int(x) for x in np.cumsum(self.sizes)]
        self.B = self.row_start[-1]
        self.cloud_shape = shapes[0]
        self.device = self.parts[0].device
        self._stage = {}
        self._copy_stream = None

    def refresh(self):
        """every part's sync_writes(): call it after the host buffers were written"""
        return sum(d.sync_writes() for d in self.parts)

    def _draw(self, batch_size, rng, batch_idx):
        if batch_size is not None and int(batch_size) != self.B:
            raise ValueError("MixedDeviceReplay draws %d rows (%s), not %d" % (self.B, self.sizes, int(batch_size)))
        if batch_idx is None:
            idx = [d.memory.draw_indices(n, rng) for d, n in zip(self.parts, self.sizes)]          # list order: expert first
        else:
            if len(batch_idx) != len(self.parts):
                raise ValueError("MixedDeviceReplay: batch_idx needs one index array per part")
            idx = list(batch_idx)
        idx = [np.asarray(i, dtype=np.int64).reshape(-1) for i in idx]
        if [len(i) for i in idx] != self.sizes:
            raise ValueError("MixedDeviceReplay: index arrays of %s rows for parts of %s" % ([len(i) for i in idx], self.sizes))
        return idx

    def _stage_indices(self, idx):
        it = _take_stage_set(self._stage, self.B, self.device, self.RING)
        h, g = it["host"].numpy(), it["ghost"].numpy()
        relabel = False
        on_device = [False] * len(self.parts)    # parts whose hindsight goals are formed behind the gather
        for s, (d, ix, lo, hi) in enumerate(zip(self.parts, idx, self.row_start[:-1], self.row_start[1:])):
            if hi == lo:
                continue
            m = d.memory
            h[0, lo:hi], h[1, lo:hi], h[2, lo:hi] = ix, m.next_indices(ix), m.episode_map[ix]
            if d._relabels() and d.relabel == "device":
                on_device[s] = True
            elif d._relabels():                  # hindsight goals of this part's on-policy rows
                if not relabel:
                    g[:, 7] = 0.0                # every other row keeps its stored goal
                    relabel = True
                mask, goal, _ = m.onpolicy_goals(ix)
                g[lo:hi, :7] = goal
                g[lo:hi, 7] = np.asarray(mask, dtype=np.float32).reshape(-1)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        _upload_stage_set(it, self._copy_stream, [d._ev_refresh for d in self.parts], relabel)
        it["relabel_device"] = on_device if any(on_device) else None
        return it

    def _handle(self, idx, it):
        dev = it["dev"]
        counts = sum(d._mask_counts(ix) for d, ix in zip(self.parts, idx))
        return {"replay_gather": self, "idx": dev[0], "nxt": dev[1], "end": dev[2], "ready_event": it["copied"], "_stage_set": it,
                "relabel_mode": tuple(d.relabel for d in self.parts), "batch_idx": np.concatenate([np.uint8(ix) for ix in idx]),
                "point_state_batch": _Shape((self.B,) + self.cloud_shape),
                "mask_counts": counts}

    def sample_lazy(self, batch_size=None, rng=None, batch_idx=None):
        """a handle for FusedRuntime.upload (DeviceReplay.sample_lazy's contract); batch_size: None or the total B;
        batch_idx: one index array per part"""
        idx = self._draw(batch_size, rng, batch_idx)
        return self._handle(idx, self._stage_indices(idx))

    def gather_into(self, lazy, dbuf):
        """fill the runtime's static batch buffers from a sample_lazy() handle: one launch, ordered on the CURRENT stream after
        the handle's index upload"""
        cur = torch.cuda.current_stream()
        if lazy.get("ready_event") is not None:
            cur.wait_event(lazy["ready_event"])
        it = lazy.get("_stage_set")
        a = hip.ReplayMixArgs()
        a.B, a.n_src = self.B, len(self.parts)
        a.cloud_elems = int(self.cloud_shape[0] * self.cloud_shape[1])
        for s, r in enumerate(self.row_start):
            a.row_start[s] = r
        for s, (d, n) in enumerate(zip(self.parts, self.sizes)):
            if n == 0:
                continue                         # owns no row: stays NULL, never read
            src = a.src[s]
            src.point_state, src.timestep = hip.ptr(d.point_state), hip.ptr(d.timestep)
            for name in ("action", "expert_action", "goal", "reward", "returns", "terminal", "expert_flags", "perturb_flags"):
                setattr(src, name, hip.ptr(d.rows[name]))
        a.idx, a.nxt, a.end = hip.ptr(lazy["idx"]), hip.ptr(lazy["nxt"]), hip.ptr(lazy["end"])
        if it is not None and it.get("relabel"):
            a.relabel = hip.ptr(it["gdev"])
        a.out_point, a.out_next_point = hip.ptr(dbuf["point_state_batch"]), hip.ptr(dbuf["next_point_state_batch"])
        for dst, key in (("out_action", "action_batch"), ("out_expert_action", "expert_action_batch"), ("out_goal", "goal_batch"),
                         ("out_reward", "reward_batch"), ("out_return", "return_batch"), ("out_mask", "mask_batch"),
                         ("out_time", "time_batch"), ("out_time_m1", "time_m1"), ("out_expert_flag", "expert_flag_batch"),
                         ("out_perturb_flag", "perturb_flag_batch")):
            setattr(a, dst, hip.ptr(dbuf[key]))
        hip.call_struct("gad_replay_gather_multi", a)
        if it is not None and it.get("relabel_device"):      # reads idx / end of the set's device block: before `used` records
            _launch_relabel(self.B, self.row_start, [(d.state_pose, d.rows["expert_flags"]) if on else None
                                                     for d, on in zip(self.parts, it["relabel_device"])],
                            lazy["idx"], lazy["end"], dbuf["goal_batch"])
        if it is not None:
            _stage_set_used(it, cur)

    def release(self, lazy):
        """give back the staging set of a handle that will never reach an update step (DeviceReplay.release)"""
        it = lazy.get("_stage_set") if isinstance(lazy, dict) else None
        if it is not None:
            it["pending"] = False

    def sample(self, batch_size=None, rng=None, batch_idx=None):
        """the update step's 11 arrays as CUDA float32 tensors of B rows (DeviceReplay.sample's layout) + `batch_idx` and
        `mask_counts`: the same one launch, into fresh tensors"""
        idx = self._draw(batch_size, rng, batch_idx)
        lazy = self._handle(idx, self._stage_indices(idx))
        B, f32 = self.B, dict(dtype=torch.float32, device=self.device)
        out = {"point_state_batch": torch.empty((B,) + self.cloud_shape, **f32),
               "next_point_state_batch": torch.empty((B,) + self.cloud_shape, **f32),
               "action_batch": torch.empty(B, 6, **f32), "expert_action_batch": torch.empty(B, 6, **f32),
               "goal_batch": torch.empty(B, 7, **f32), "time_m1": torch.empty(B, **f32)}
        for k in ("reward_batch", "return_batch", "mask_batch", "time_batch", "expert_flag_batch", "perturb_flag_batch"):
            out[k] = torch.empty(B, **f32)
        self.gather_into(lazy, out)
        del out["time_m1"]
        out["batch_idx"], out["mask_counts"] = lazy["batch_idx"], lazy["mask_counts"]
        return out
