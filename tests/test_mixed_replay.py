"""Host side of the two-buffer minibatch (reference core/trainer.py:212-232: expert rows + online rows, concatenated key by
key): replay_memory.sample_mixed against a restatement of the reference's dict comprehension, the written-slot arithmetic
behind DeviceReplay.sync_writes against the slots push() really wrote, and the C boundary of gad_replay_gather_multi --
struct sizes and every host-side refusal.  No GPU: nothing here launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ga_ddpg_amd.core.replay_memory import BaseMemory, sample_mixed, written_slots
from ga_ddpg_amd.experiments.config import load_cfg
from ga_ddpg_amd.synth_data import fill_synthetic_buffer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def buffers():
    cfg = load_cfg("ddpg_td3_aux.yaml")
    expert = BaseMemory(300, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(expert, 300, seed=21)
    online = BaseMemory(170, cfg, name="online", point_dtype=np.float32)
    fill_synthetic_buffer(online, 150, seed=22)
    return expert, online


def _reference_concat(batch_data, online_batch_data):
    """the learner's rule, restated (reference core/trainer.py:218-219)"""
    return {k: np.concatenate((batch_data[k], online_batch_data[k]), axis=0) for k in batch_data.keys()
            if type(batch_data[k]) is np.ndarray and k in online_batch_data.keys()}


@pytest.mark.parametrize("sizes", [(5, 3), (5, 0), (0, 3)])
def test_sample_mixed_is_the_reference_concatenation(buffers, sizes):
    expert, online = buffers
    idx = [expert.draw_indices(sizes[0], np.random.default_rng(1)), online.draw_indices(sizes[1], np.random.default_rng(2))]
    want = _reference_concat(expert.sample(sizes[0], batch_idx=idx[0]), online.sample(sizes[1], batch_idx=idx[1]))
    got = sample_mixed((expert, online), sizes, batch_idx=idx)
    first = expert.sample(sizes[0], batch_idx=idx[0])
    assert set(got) == {k for k, v in first.items() if type(v) is np.ndarray} and len(got) == 22
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got[k].shape[0] == (0 if k == "grasp_sample_batch" else sum(sizes)), k     # (that key is an empty (0, 4, 4) array)
    # expert rows first
    np.testing.assert_array_equal(got["action_batch"][:sizes[0]], expert.action[idx[0]])
    np.testing.assert_array_equal(got["action_batch"][sizes[0]:], online.action[idx[1]])
    # one generator: expert drawn first, then online, from the same stream
    r1, r2 = np.random.default_rng(7), np.random.default_rng(7)
    a = expert.sample(sizes[0], rng=r2)
    b = online.sample(sizes[1], rng=r2)
    got = sample_mixed((expert, online), sizes, rng=r1)
    want = _reference_concat(a, b)
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="rng " + k)
    assert r1.integers(0, 1 << 30) == r2.integers(0, 1 << 30)          # ... and both consumed the same amount of it


def test_sample_mixed_takes_no_rows_from_a_relabelling_buffer(buffers):
    """size 0 on a buffer that relabels its goals (self_supervision, not the expert buffer): an empty batch keeps its columns"""
    expert, online = buffers
    online.self_supervision = True
    try:
        got = sample_mixed((expert, online), (4, 0), rng=np.random.default_rng(3))
        only = online.sample(0)
    finally:
        online.self_supervision = False
    assert only["goal_batch"].shape == (0, 7) and only["next_goal_batch"].shape == (0, 7)
    assert got["goal_batch"].shape == (4, 7) and got["point_state_batch"].shape[0] == 4


def test_sample_mixed_argument_checks(buffers):
    expert, online = buffers
    with pytest.raises(ValueError):
        sample_mixed((expert, online), (4,))
    with pytest.raises(ValueError):
        sample_mixed((expert, online), (4, 4), batch_idx=[np.arange(30, 34)])


def _push_n(mem, n, tag):
    """n pushes, each cloud filled with its own tag; -> the next unused tag"""
    shape = mem.point_state.shape[1:]
    for _ in range(n):
        mem.push({"point_state": np.full(shape, float(tag), dtype=np.float32), "reward": 0.0, "timestep": float(tag % 7)})
        tag += 1
    return tag


@pytest.mark.parametrize("start", [0, 5])
def test_written_slots_are_the_slots_push_wrote(start, tmp_path):
    cfg = load_cfg("ddpg_td3_aux.yaml")
    cap = 64
    mem = BaseMemory(cap, cfg, name="online", point_dtype=np.float32)
    mem.buffer_start_idx = start
    tag = 1
    # (pushes, explained by pushes alone?): no wrap; up to the last slot; across the end; a whole lap; nothing; more than a lap
    for n, explained in ((10, True), (50, True), (3, True), (10, True), (cap, True), (0, True), (cap + 1, False), (7, True)):
        before, s0 = mem.point_state.copy(), mem.write_stamp()
        tag = _push_n(mem, n, tag)
        got = written_slots(s0, mem.write_stamp(), cap, start)
        changed = np.flatnonzero((mem.point_state != before).any(axis=(1, 2)))
        if not explained:
            assert got is None, (n, got)
            continue
        assert got is not None and got.dtype == np.int64, n
        np.testing.assert_array_equal(got, changed, err_msg="%d pushes from stamp %s" % (n, s0))
    assert mem.is_full
    # a dropped frame (empty cloud) moves nothing
    s0 = mem.write_stamp()
    mem.push({"point_state": np.zeros(mem.point_state.shape[1:], dtype=np.float32)})
    assert len(written_slots(s0, mem.write_stamp(), cap, start)) == 0
    # reset() and load() are not pushes: everything may have changed
    s0 = mem.write_stamp()
    mem.reset()
    assert written_slots(s0, mem.write_stamp(), cap, start) is None
    _push_n(mem, 30, tag)                                             # (a saved file's episode_map decides how much load() reads)
    mem.episode_map[:30] = 29
    mem.save(str(tmp_path))
    s0 = mem.write_stamp()
    mem.load(str(tmp_path))
    assert written_slots(s0, mem.write_stamp(), cap, start) is None
    assert written_slots(None, mem.write_stamp(), cap, start) is None
    # arrays written behind push()'s back announce themselves
    s0 = mem.write_stamp()
    fill_synthetic_buffer(mem, 40, seed=3)
    assert written_slots(s0, mem.write_stamp(), cap, start) is None


def test_mix_args_mirror_the_header():
    from ga_ddpg_amd import hip
    src = '#include "gaddpg.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %d %zu %zu %zu\\n", ' \
          'sizeof(gad_replay_mix_args), sizeof(gad_replay_src), GAD_REPLAY_MAX_SRC, offsetof(gad_replay_mix_args, src), ' \
          'offsetof(gad_replay_mix_args, relabel), offsetof(gad_replay_mix_args, out_perturb_flag));return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(hip.ReplayMixArgs), C.sizeof(hip.ReplaySrc), hip.REPLAY_MAX_SRC, hip.ReplayMixArgs.src.offset,
                   hip.ReplayMixArgs.relabel.offset, hip.ReplayMixArgs.out_perturb_flag.offset]
    assert C.sizeof(hip.ReplaySrc) == 80 and "gad_replay_gather_multi" in hip.EXPORTS


SRC_FIELDS = ["point_state", "action", "expert_action", "goal", "reward", "returns", "terminal", "timestep", "expert_flags",
              "perturb_flags"]
OUT_FIELDS = ["out_point", "out_action", "out_expert_action", "out_goal", "out_reward", "out_return", "out_mask", "out_time",
              "out_time_m1", "out_expert_flag", "out_perturb_flag"]


def _valid_args(hip, rows=(2, 3)):
    """arguments that pass every host-side check (dummy non-NULL addresses: never handed to a launch here)"""
    a = hip.ReplayMixArgs()
    a.B, a.cloud_elems, a.n_src = sum(rows), 8, len(rows)
    for s, r in enumerate(np.cumsum((0,) + tuple(rows))):
        a.row_start[s] = int(r)
    for s, n in enumerate(rows):
        if n:
            for f in SRC_FIELDS:
                setattr(a.src[s], f, 0x1000)
    for f in ["idx", "nxt", "end", "out_next_point"] + OUT_FIELDS:
        setattr(a, f, 0x1000)
    return a


def test_gather_multi_refuses_bad_arguments_before_any_launch():
    """every refusal is the ONLY defect of otherwise valid arguments, so each check is shown to exist; a status < 0 with a
    message, and no launch (this runs without a GPU)"""
    from ga_ddpg_amd import hip
    L = hip.lib()
    null = C.c_void_p(None)
    ERR_NULL, ERR_SHAPE = -1, -2

    def refused(a, status, word):
        rc = L.gad_replay_gather_multi(C.byref(a), null)
        msg = L.gad_last_error()
        assert rc == status and b"replay_gather_multi" in msg and word in msg, (rc, msg, word)

    rc = L.gad_replay_gather_multi(null, null)
    assert rc == ERR_NULL and b"replay_gather_multi" in L.gad_last_error()
    for n_src in (0, 5, -1):
        a = _valid_args(hip)
        a.n_src = n_src
        refused(a, ERR_SHAPE, b"n_src")
    a = _valid_args(hip)
    a.row_start[0] = 1
    refused(a, ERR_SHAPE, b"row_start")
    a = _valid_args(hip)
    a.row_start[2] = 4                                                 # does not end at B = 5
    refused(a, ERR_SHAPE, b"row_start")
    a = _valid_args(hip, rows=(2, 2, 1))
    a.row_start[1], a.row_start[2] = 3, 2                              # 0, 3, 2, 5: decreasing
    refused(a, ERR_SHAPE, b"decreases")
    for B in (0, -3):
        a = _valid_args(hip)
        a.B = B
        a.row_start[1] = a.row_start[2] = B
        refused(a, ERR_SHAPE, b"B ")
    for ce in (7, 0, 1, -2):
        a = _valid_args(hip)
        a.cloud_elems = ce
        refused(a, ERR_SHAPE, b"cloud_elems")
    for f in SRC_FIELDS:                                               # a NULL pointer in a source that owns rows
        for s in (0, 1):
            a = _valid_args(hip)
            setattr(a.src[s], f, None)
            refused(a, ERR_NULL, b"source %d" % s)
    for f in OUT_FIELDS:
        a = _valid_args(hip)
        setattr(a, f, None)
        refused(a, ERR_NULL, b"output")
    for f in ("idx", "nxt", "end"):
        a = _valid_args(hip)
        setattr(a, f, None)
        refused(a, ERR_NULL, b"index")
    with pytest.raises(RuntimeError, match="gad_replay_gather_multi failed"):
        hip.check(L.gad_replay_gather_multi(C.byref(hip.ReplayMixArgs()), null), "gad_replay_gather_multi")
    # the plan table knows the entry (tests/test_abi.py checks the whole table against the header)
    names = {L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())}
    assert "gad_replay_gather_multi" in names and L.gad_abi_version() == 12
