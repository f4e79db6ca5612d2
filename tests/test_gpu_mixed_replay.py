"""The two-buffer minibatch on the GPU (reference core/trainer.py:212-232: batch_size expert rows + int(batch_size *
online_buffer_ratio) online rows, expert first): gad_replay_gather_multi bit-exact against numpy, MixedDeviceReplay against
replay_memory.sample_mixed, one DDPG update on either feed, train_off_policy(online_memory=...) on both feeding paths, and
DeviceReplay.sync_writes.  Copies and selections: bit-exact (assert_array_equal / bit patterns).  The update's outputs: the
tolerance tests/test_gpu_modules.py::test_device_replay_matches_host_sampling uses for the same comparison (same inputs,
run-to-run atomics noise only)."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.test_gpu_optim_kernels import Buf, _nan32, _same

pytestmark = pytest.mark.gpu

CAPS = (5, 3, 7, 4)                  # capacities differ between the sources
SRC_FIELDS = {"point_state": None, "action": 6, "expert_action": 6, "goal": 7, "reward": 0, "returns": 0, "terminal": 0,
              "timestep": 0, "expert_flags": 0, "perturb_flags": 0}
OUTS = {"out_point": "point_state", "out_next_point": "point_state", "out_action": "action", "out_expert_action": "expert_action",
        "out_goal": "goal", "out_reward": "reward", "out_return": "returns", "out_mask": "terminal", "out_time": None,
        "out_time_m1": None, "out_expert_flag": "expert_flags", "out_perturb_flag": "perturb_flags"}


def _hip():
    from ga_ddpg_amd import hip
    return hip


def _tag(k, *shape):
    return (k * 1000.0 + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) * 0.25 + 0.125).astype(np.float32)


def _source(s, cap, cloud_elems, rng):
    """buffer s: every field tagged with its source and field number, so a row taken from the wrong source or field shows"""
    src = {}
    for f, (name, w) in enumerate(SRC_FIELDS.items()):
        shape = (cap, cloud_elems) if w is None else ((cap, w) if w else (cap,))
        src[name] = _tag(20 * (s + 1) + f, *shape)
    t = rng.integers(0, 30, cap).astype(np.float32)
    t[:3] = [1e8, 3.0, 16777216.0]                                      # t[end] + 1 rounds before t[idx] is subtracted
    src["timestep"] = t
    return src


def _local_indices(s, cap, n, rng):
    """first row of a source: local index 0 (the same in every source); last row: cap - 1; in between the rounding case
    (idx 2, end 0), a repeat of index 0, then random ones.  A one-row source takes 0 or cap - 1 in turn."""
    idx = rng.integers(0, cap, n).astype(np.int64)
    end = rng.integers(0, cap, n).astype(np.int64)
    if n == 1:
        idx[0] = 0 if s % 2 == 0 else cap - 1
    elif n >= 2:
        idx[0], idx[-1] = 0, cap - 1
        end[-1] = cap - 1                                               # end == idx
        if n >= 3:
            idx[1], end[1] = 2, 0                                       # float32(1e8 + 1) - 16777216
        if n >= 4:
            idx[2] = 0                                                  # a repeated index
    return idx, (idx + 1) % cap, end                                    # the successor wraps to 0 at cap - 1


def _relabel_block(rows, rng):
    """(B, 8): flags > 0 on the rows either side of every boundary (and the first and last row), 0 / negative / NaN elsewhere"""
    B = sum(rows)
    g = _tag(99, B, 8)
    flags = rng.choice(np.array([0.0, -1.0, -0.0, np.nan], np.float32), B)
    edge = {0, B - 1}
    for r in np.cumsum(rows)[:-1]:
        edge |= {int(r) - 1, int(r)}
    for j, b in enumerate(sorted(e for e in edge if 0 <= e < B)):
        flags[b] = (1.0, 0.5, 1e-30)[j % 3]
    g[:, 7] = flags
    return g


def _run_multi(rows, cloud_elems, with_next, relabel, shift, seed):
    """-> (got, want): the kernel's outputs and numpy's, for a split `rows` over the first len(rows) sources"""
    hip = _hip()
    rng = np.random.default_rng(seed)
    B = sum(rows)
    srcs = [_source(s, CAPS[s], cloud_elems, rng) for s in range(len(rows))]
    loc = [_local_indices(s, CAPS[s], n, rng) for s, n in enumerate(rows)]
    idx, nxt, end = (np.concatenate([l[k] for l in loc]) for k in range(3))
    # shift 8: every cloud pointer, sources and outputs, sits two floats off 16-byte alignment; "src1": only source 1's clouds
    src_shift = lambda k, s: 8 if k == "point_state" and (shift == 8 or (shift == "src1" and s == 1)) else 0
    out_shift = lambda k: 8 if k in ("out_point", "out_next_point") and shift == 8 else 0
    bs = [{k: Buf(v, shift=src_shift(k, s)) for k, v in src.items()} if rows[s] else None for s, src in enumerate(srcs)]
    bi = {"idx": Buf(idx), "nxt": Buf(nxt), "end": Buf(end)}
    shapes = {k: ((B, cloud_elems) if v == "point_state" else ((B, SRC_FIELDS[v]) if v and SRC_FIELDS[v] else (B,)))
              for k, v in OUTS.items()}
    bo = {k: Buf(_nan32(int(np.prod(sp))).reshape(sp), shift=out_shift(k)) for k, sp in shapes.items()}
    g = _relabel_block(rows, rng) if relabel else None
    bg = Buf(g) if relabel else None
    a = hip.ReplayMixArgs()
    a.B, a.cloud_elems, a.n_src = B, cloud_elems, len(rows)
    for s, r in enumerate(np.cumsum((0,) + tuple(rows))):
        a.row_start[s] = int(r)
    for s, b in enumerate(bs):
        if b is not None:                                               # a source without rows stays all NULL
            for k, buf in b.items():
                setattr(a.src[s], k, buf.ptr)
    for k, b in list(bi.items()) + list(bo.items()):
        setattr(a, k, b.ptr)
    if not with_next:
        a.out_next_point = None
    if relabel:
        a.relabel = bg.ptr
    hip.call_struct("gad_replay_gather_multi", a)
    want = {k: np.full(s, np.nan, np.float32) for k, s in shapes.items()}
    for s, n in enumerate(rows):
        lo = int(a.row_start[s])
        src, (i, nx, e) = srcs[s], loc[s]
        t = src["timestep"]
        tm = ((t[e] + np.float32(1)).astype(np.float32) - t[i]).astype(np.float32)           # the kernel's order of operations
        for k, f in OUTS.items():
            if k == "out_time":
                want[k][lo:lo + n] = tm
            elif k == "out_time_m1":
                want[k][lo:lo + n] = (tm - np.float32(1)).astype(np.float32)
            elif k == "out_next_point":
                if with_next:
                    want[k][lo:lo + n] = src[f][nx]
            else:
                want[k][lo:lo + n] = src[f][i]
    if relabel:
        with np.errstate(invalid="ignore"):
            want["out_goal"] = np.where(g[:, 7:8] > 0, g[:, :7], want["out_goal"])           # DeviceReplay._apply_relabel
    got = {k: bo[k].get(k) for k in OUTS}                               # (Buf.get checks the guard bytes too)
    for s, b in enumerate(bs):
        if b is not None:
            for k, buf in b.items():
                _same("source %d %s untouched" % (s, k), buf.get(), srcs[s][k])
    if relabel:
        _same("relabel block untouched", bg.get(), g)
    return got, want


def _check(rows, cloud_elems, with_next, relabel, shift, seed):
    got, want = _run_multi(rows, cloud_elems, with_next, relabel, shift, seed)
    for k in OUTS:
        _same("gather_multi rows %s cloud %d next %d relabel %d shift %s: %s" % (rows, cloud_elems, with_next, relabel, shift, k),
              got[k], want[k])


SPLITS = [(1,), (2, 3), (1, 0), (0, 1), (3, 0, 2), (1, 1, 1, 1), (4, 5, 0, 3)]
CASES = [(rows, shift) for rows in SPLITS for shift in (0, 8)] + [((2, 3), "src1"), ((1, 1, 1, 1), "src1")]


@pytest.mark.parametrize("rows,shift", CASES)
def test_gather_multi_bit_exact(rows, shift):
    seed = 4000 + 17 * SPLITS.index(rows)
    for cloud_elems in (2, 6, 8, 4120):
        for with_next in (True, False):
            for relabel in (False, True):
                _check(rows, cloud_elems, with_next, relabel, shift, seed + cloud_elems)


@pytest.mark.parametrize("shift", (0, 8))
@pytest.mark.parametrize("relabel", (False, True))
def test_gather_multi_bit_exact_128_128(shift, relabel):
    """the shipped configuration's batch: 128 + 128 rows of 4 x 1030 floats"""
    _check((128, 128), 4120, True, relabel, shift, 4500)


@pytest.mark.parametrize("cloud_elems", (6, 8, 4120))
def test_gather_multi_single_source_equals_replay_gather(cloud_elems):
    hip = _hip()
    rng = np.random.default_rng(4600 + cloud_elems)
    B, cap = 9, 7
    src = _source(0, cap, cloud_elems, rng)
    idx, nxt, end = _local_indices(0, cap, B, rng)
    bs = {k: Buf(v) for k, v in src.items()}
    bi = {"idx": Buf(idx), "nxt": Buf(nxt), "end": Buf(end)}
    shapes = {k: ((B, cloud_elems) if v == "point_state" else ((B, SRC_FIELDS[v]) if v and SRC_FIELDS[v] else (B,)))
              for k, v in OUTS.items()}
    outs = []
    for multi in (False, True):
        bo = {k: Buf(_nan32(int(np.prod(s))).reshape(s)) for k, s in shapes.items()}
        a = hip.ReplayMixArgs() if multi else hip.ReplayGatherArgs()
        a.B, a.cloud_elems = B, cloud_elems
        if multi:
            a.n_src, a.row_start[1] = 1, B
        for k, b in bs.items():
            setattr(a.src[0] if multi else a, k, b.ptr)
        for k, b in list(bi.items()) + list(bo.items()):
            setattr(a, k, b.ptr)
        hip.call_struct("gad_replay_gather_multi" if multi else "gad_replay_gather", a)
        outs.append({k: bo[k].get(k) for k in OUTS})
    for k in OUTS:
        assert not np.isnan(outs[0][k]).any(), k
        _same("one source vs gad_replay_gather: " + k, outs[1][k], outs[0][k])


# ----------------------------------------------------------------------------- MixedDeviceReplay
def _rigid_poses(mem, seed):
    """proper rigid poses, so the relabelled goals are well defined (as tests/test_gpu_modules.py builds them)"""
    rng = np.random.default_rng(seed)
    for i in range(mem.state_pose.shape[0]):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        mem.state_pose[i] = np.eye(4)
        mem.state_pose[i][:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        mem.state_pose[i][:3, 3] = rng.normal(size=3)


def _two_buffers(cfg, relabel=False, online_cap=200, online_fill=170):
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    expert = BaseMemory(400, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(expert, 400, seed=31)
    online = BaseMemory(online_cap, cfg, name="online", point_dtype=np.float32)
    fill_synthetic_buffer(online, online_fill, seed=32)
    if relabel:
        online.self_supervision = True
        _rigid_poses(online, 2)
    return expert, online


def _f32(host, k, like):
    return np.asarray(host[k], dtype=np.float32).reshape(like.shape)


def _valid(batch):
    """the masked means of the update are defined: an expert row, a positive return, an unperturbed row"""
    return (batch["expert_flag_batch"] >= 1).any() and (batch["return_batch"] > 0).any() and (batch["perturb_flag_batch"] < 1).any()


@pytest.mark.parametrize("relabel", (False, True))
def test_mixed_device_replay_matches_sample_mixed(relabel):
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.device_replay import DeviceReplay, MixedDeviceReplay
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    from ga_ddpg_amd.parallel import mask_counts
    from ga_ddpg_amd.runtime import BATCH_KEYS
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    expert, online = _two_buffers(cfg, relabel)
    d0, d1 = DeviceReplay(expert), DeviceReplay(online)
    rt, both_kinds = None, 0
    for sizes in ((5, 3), (8, 0), (0, 8)):
        mixed = MixedDeviceReplay([(d0, sizes[0]), (d1, sizes[1])])
        assert mixed.B == 8
        for trial in range(2):
            idx = [expert.draw_indices(sizes[0], np.random.default_rng(40 + trial)),
                   online.draw_indices(sizes[1], np.random.default_rng(50 + trial))]
            if trial == 0 and sizes[1] >= 2:                           # on-policy and expert rows of the online buffer, in turn
                hi = online.upper_idx()
                kinds = [np.flatnonzero(online.expert_flags[:hi] == 0), np.flatnonzero(online.expert_flags[:hi] != 0)]
                idx[1] = np.array([kinds[j % 2][(7 * j) % len(kinds[j % 2])] for j in range(sizes[1])], dtype=np.int64)
            host = sample_mixed((expert, online), sizes, batch_idx=idx)
            flags = online.expert_flags[idx[1]]
            if relabel and (flags == 0).any() and (flags != 0).any():  # relabelled and unrelabelled online rows in one batch
                both_kinds += 1
                assert np.abs(host["goal_batch"][sizes[0]:] - online.goal[idx[1]]).max() > 1e-3
            np.testing.assert_array_equal(host["goal_batch"][:sizes[0]], expert.goal[idx[0]])       # expert rows keep their goals
            dev = mixed.sample(batch_idx=idx)
            np.testing.assert_array_equal(dev["batch_idx"], host["batch_idx"])
            np.testing.assert_array_equal(dev["mask_counts"], mask_counts(host))
            for k in BATCH_KEYS:
                np.testing.assert_array_equal(dev[k].cpu().numpy(), _f32(host, k, dev[k]), err_msg="eager %s %s" % (sizes, k))
            lazy = mixed.sample_lazy(batch_idx=idx)
            assert lazy["replay_gather"] is mixed and lazy["point_state_batch"].shape == (8,) + tuple(expert.point_state.shape[1:])
            np.testing.assert_array_equal(lazy["batch_idx"], host["batch_idx"])
            np.testing.assert_array_equal(lazy["mask_counts"], mask_counts(host))
            rt = rt or agent.runtime(8, expert.point_state.shape[2])
            rt.upload(lazy)
            torch.cuda.synchronize()
            for k in BATCH_KEYS:
                np.testing.assert_array_equal(rt.dbuf[k].cpu().numpy(), _f32(host, k, rt.dbuf[k]), err_msg="lazy %s %s" % (sizes, k))
            np.testing.assert_array_equal(rt.dbuf["time_m1"].cpu().numpy(), np.asarray(host["time_batch"], dtype=np.float32) - 1.0)
        # one rng: expert indices first, then online, as sample_mixed draws them
        lazy = mixed.sample_lazy(8, rng=np.random.default_rng(6))
        np.testing.assert_array_equal(lazy["batch_idx"], sample_mixed((expert, online), sizes, rng=np.random.default_rng(6))["batch_idx"])
        mixed.release(lazy)
        # handles drawn ahead by a prefetcher and never consumed give their staging sets back
        for _ in range(12):
            with PrefetchSampler(mixed, 8, depth=3, rng=np.random.default_rng(0)) as s:
                mixed.release(s.next())
        sets = mixed._stage[("sets", 8)]["items"]
        assert sum(1 for it in sets if it is not None and it["pending"]) <= 2, "leaked staging sets"
    assert both_kinds >= 2 or not relabel                              # (the crafted batches of sizes (5, 3) and (0, 8))
    with pytest.raises(ValueError):
        mixed.sample_lazy(7)
    with pytest.raises(ValueError):
        MixedDeviceReplay([(d0, 1)] * 5)


def test_mixed_device_replay_refuses_unequal_clouds():
    from ga_ddpg_amd.core.device_replay import DeviceReplay, MixedDeviceReplay
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.experiments.config import load_cfg
    cfg = load_cfg("ddpg_td3_aux.yaml")
    a = BaseMemory(40, cfg, point_dtype=np.float32)
    b = BaseMemory(40, cfg, name="online", point_dtype=np.float32)
    b.point_state = np.zeros((40, 4, a.point_state.shape[2] - 2), dtype=np.float32)
    with pytest.raises(ValueError, match="different shapes"):
        MixedDeviceReplay([(DeviceReplay(a), 4), (DeviceReplay(b), 4)])


def test_update_on_a_mixed_lazy_batch_equals_the_host_batch():
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.device_replay import DeviceReplay, MixedDeviceReplay
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    from ga_ddpg_amd.runtime import BATCH_KEYS
    from oracle.detfill import fill_module_
    agents = []
    for _ in range(2):
        a, cfg = make_agent("ddpg_td3_aux.yaml")
        for name in ("policy", "policy_target", "critic", "critic_target", "state_feature_extractor"):
            fill_module_(getattr(a, name), name, 7)
        agents.append(a)
    expert, online = _two_buffers(cfg)
    mixed = MixedDeviceReplay([(DeviceReplay(expert), 12), (DeviceReplay(online), 12)])
    idx = [expert.draw_indices(12, np.random.default_rng(3)), online.draw_indices(12, np.random.default_rng(4))]
    host = sample_mixed((expert, online), (12, 12), batch_idx=idx)
    assert _valid(host)                                                # (a property of the seeded buffers, not of the code under test)
    lazy = mixed.sample_lazy(batch_idx=idx)
    u = np.random.default_rng(5).random((24, 6)).astype(np.float32)
    r_host = agents[0].update_parameters(host, agents[0].update_step, 0, noise_u=u)
    r_dev = agents[1].update_parameters(lazy, agents[1].update_step, 0, noise_u=u)
    assert set(r_dev) == set(r_host) and len(r_host) > 3
    for k in r_host:
        assert_close(r_dev[k], r_host[k], 2e-3, 1e-6, k)               # same inputs; run-to-run atomics noise only
    torch.cuda.synchronize()
    rt = agents[1].runtime(24, expert.point_state.shape[2])
    for k in BATCH_KEYS:
        np.testing.assert_array_equal(rt.dbuf[k].cpu().numpy(), _f32(host, k, rt.dbuf[k]), err_msg=k)


TRAIN_SEED = 0


@pytest.mark.parametrize("case", ("device", "host", "no_online_memory", "ratio_0"))
def test_train_off_policy_with_an_online_memory(case):
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    config = cfg.RL_TRAIN
    assert config.onpolicy and config.online_buffer_ratio == 1.0      # the shipped configuration
    config.batch_size, config.updates_per_step, config.max_epoch, config.save_epoch = 8, 2, 1000, []
    if case == "ratio_0":
        config.online_buffer_ratio = 0.0
    expert, online = _two_buffers(cfg)
    mixed_case = case in ("device", "host")
    if mixed_case:
        rng = np.random.default_rng(TRAIN_SEED)
        want = [sample_mixed((expert, online), (8, 8), rng=rng) for _ in range(4)]
        assert all(_valid(b) for b in want)                            # (a property of the seeded buffers and TRAIN_SEED)
        want = [b["batch_idx"] for b in want]
    else:
        rng = np.random.default_rng(TRAIN_SEED)
        want = [expert.sample(8, rng=rng)["batch_idx"] for _ in range(4)]
    seen = []
    inner = agent.update_parameters

    def recording(batch_data, *a, **kw):
        seen.append(np.array(batch_data["batch_idx"]))
        return inner(batch_data, *a, **kw)
    agent.update_parameters = recording
    logs = []
    losses, epochs = tto.train_off_policy(agent, expert, config, None, save_model=False, max_epochs=2, log=logs.append,
                                          device_replay=(case != "host"), rng=np.random.default_rng(TRAIN_SEED),
                                          online_memory=None if case == "no_online_memory" else online)
    assert epochs == 2 and len(seen) == 4
    rows = 16 if mixed_case else 8
    assert all(len(s) == rows for s in seen)
    assert any(("batch size: %d" % rows) in l for l in logs)
    for got, exp in zip(seen, want):
        np.testing.assert_array_equal(got, exp)
    if mixed_case:
        assert all(np.isfinite(list(h)).all() for h in losses.values())
        assert len(losses["critic_loss"]) == 5                          # deque([0]) + 4 updates
    if case == "device":
        assert tto.mixed_device_mirror(expert, online, 8, 8) is tto.mixed_device_mirror(expert, online, 8, 8)


# ----------------------------------------------------------------------------- sync_writes
def _rollout(mem, n, tag, reward):
    shape = mem.point_state.shape[1:]
    ep = []
    for t in range(n):
        ep.append({"point_state": np.full(shape, float(tag + t), dtype=np.float32), "action": np.full(6, 0.001 * (tag + t), np.float32),
                   "expert_action": np.full(6, -0.001 * (tag + t), np.float32), "goal": np.full(7, 0.01 * t, np.float32),
                   "reward": float(reward) if t == n - 1 else 0.0, "terminal": float(t == n - 1), "timestep": float(t),
                   "expert_flags": float(t % 2), "perturb_flags": 0.0, "target_name": "box"})
    return ep


def _mirror_equals_host(dmem, mem):
    hi = mem.upper_idx()
    np.testing.assert_array_equal(dmem.point_state[:hi].cpu().numpy(), np.asarray(mem.point_state[:hi], dtype=np.float32))
    np.testing.assert_array_equal(dmem.timestep[:hi].cpu().numpy(), np.asarray(mem.timestep[:hi], dtype=np.float32))
    for name, t in dmem.rows.items():
        np.testing.assert_array_equal(t[:hi].cpu().numpy(), np.asarray(getattr(mem, name)[:hi], dtype=np.float32), err_msg=name)


def test_sync_writes_uploads_the_written_slots_only():
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.device_replay import MixedDeviceReplay
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    from ga_ddpg_amd.experiments.config import load_cfg
    cfg = load_cfg("ddpg_td3_aux.yaml")
    expert, online = _two_buffers(cfg, online_cap=200, online_fill=185)
    online.RL = True                                                   # (add_episode keeps unsuccessful rollouts in RL mode)
    dmem = tto.device_mirror(online)
    assert dmem.uploaded_cloud_rows == 200 and dmem.sync_writes() == 0
    pushes = 0
    for n, reward in ((6, 1.0), (12, 0.0), (5, 1.0)):                  # 185 + 6 + 12 crosses the end of the buffer
        online.add_episode(_rollout(online, n, 1000 + 100 * pushes, reward))
        pushes += n
    assert online.is_full and online.cur_idx < 185
    before = dmem.uploaded_cloud_rows
    assert tto.device_mirror(online) is dmem                           # device_mirror syncs through sync_writes()
    assert dmem.uploaded_cloud_rows - before == pushes == 23
    torch.cuda.synchronize()
    _mirror_equals_host(dmem, online)
    assert dmem.sync_writes() == 0
    mixed = MixedDeviceReplay([(tto.device_mirror(expert), 5), (dmem, 6)])
    wrote = np.r_[185:200, 0:8]
    idx = [expert.draw_indices(5, np.random.default_rng(1)), wrote[[0, 5, 14, 15, 20, 22]]]
    host = sample_mixed((expert, online), (5, 6), batch_idx=idx)
    dev = mixed.sample(batch_idx=idx)
    from ga_ddpg_amd.runtime import BATCH_KEYS
    for k in BATCH_KEYS:
        np.testing.assert_array_equal(dev[k].cpu().numpy(), _f32(host, k, dev[k]), err_msg=k)
    # what pushes do not explain falls back to everything up to upper_idx()
    online.reset()
    online.add_episode(_rollout(online, 30, 5000, 1.0))
    before = dmem.uploaded_cloud_rows
    assert mixed.refresh() == online.upper_idx() == 30 and dmem.uploaded_cloud_rows - before == 30
    torch.cuda.synchronize()
    _mirror_equals_host(dmem, online)
