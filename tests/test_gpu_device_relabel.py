"""Hindsight goals formed on the device (gad_replay_relabel_goals, DeviceReplay(relabel="device")): the kernel against a float64
closed form written here, the four quaternion branches, non-finite input, the mirror classes against the host path, writes, one
DDPG update and train_off_policy(device_relabel=True).

The gate is the project's forced-decision form against float64, with the host's own BaseMemory.onpolicy_goals on the same rows
as the float32 yardstick:   err(device) <= max(3 x err(host), 2e-6),   err(x) = max |x - f64| over quaternion and translation.
Where the float64 w is below 1e-3 the quaternion's sign is determined on neither side (w >= 0 is decided by rounding) and the
quaternion is compared as min(|q - r|, |q + r|); no row is left out.  Rows the kernel must not touch are compared bit for bit."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.test_gpu_optim_kernels import Buf, _same

pytestmark = pytest.mark.gpu

ROW_START = (0, 29, 52, 67, 67)      # sources 0 and 2 relabel, source 1 has rows but no poses, source 3 has no rows
CAP = 96


def _hip():
    from ga_ddpg_amd import hip
    return hip


# ----------------------------------------------------------------------------- float64 reference
def _rot64(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return _rot64(np.r_[np.cos(angle / 2), np.sin(angle / 2) * axis])


def _quat64(R):
    """closed form in float64: divide by the largest of the four candidate components; unit length, w >= 0"""
    c = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2],
                  1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(c))
    v = [np.array([c[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]),
         np.array([R[2, 1] - R[1, 2], c[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]]),
         np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], c[2], R[1, 2] + R[2, 1]]),
         np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], c[3]])][k]
    q = v / (2.0 * np.sqrt(c[k]))
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _goal64(A, E):
    """[quaternion | translation] of inv(A) @ E, all in float64, from the float32 poses as stored"""
    M = np.linalg.inv(np.asarray(A, dtype=np.float64)) @ np.asarray(E, dtype=np.float64)
    return np.r_[_quat64(M[:3, :3]), M[:3, 3]]


def _goals64(poses, idx, end):
    return np.array([_goal64(poses[i], poses[e]) for i, e in zip(idx, end)]).reshape(len(idx), 7)


def _err(got, ref):
    """max |got - ref| over quaternion and translation; rows whose float64 w < 1e-3 compare the quaternion up to its sign"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1, 7), np.asarray(ref, dtype=np.float64).reshape(-1, 7)
    dq = np.abs(got[:, :4] - ref[:, :4]).max(axis=1)
    free = ref[:, 0] < 1e-3
    dq[free] = np.minimum(dq, np.abs(got[:, :4] + ref[:, :4]).max(axis=1))[free]
    return float(max(dq.max(), np.abs(got[:, 4:] - ref[:, 4:]).max()))


def _gate(what, dev, host, ref):
    """the gate of the module docstring on the rows given (all of them relabelled), plus w >= 0 and unit length"""
    dev = np.asarray(dev, dtype=np.float64).reshape(-1, 7)
    e_dev, e_host = _err(dev, ref), _err(host, ref)
    print("%s: %d rows, err(device) %.3g, err(host) %.3g, rows with f64 w < 1e-3: %d" % (
        what, len(dev), e_dev, e_host, int((np.asarray(ref).reshape(-1, 7)[:, 0] < 1e-3).sum())))
    assert (dev[:, 0] >= 0).all(), what
    assert np.abs(np.linalg.norm(dev[:, :4], axis=1) - 1.0).max() <= 1e-6, what
    assert e_dev <= max(3 * e_host, 2e-6), "%s: err(device) %.3g > max(3 x err(host) %.3g, 2e-6)" % (what, e_dev, e_host)


# ----------------------------------------------------------------------------- inputs
def _rigid(n, rng):
    """(n, 4, 4) float32 rigid poses: uniform rotations, unit-normal translations (as tests/test_gpu_modules.py builds them)"""
    P = np.zeros((n, 4, 4), dtype=np.float32)
    for i in range(n):
        P[i] = np.eye(4)
        P[i, :3, :3] = _rot64(rng.normal(size=4))
        P[i, :3, 3] = rng.normal(size=3)
    return P


def _rigid_poses(mem, seed):
    mem.state_pose[:] = _rigid(mem.state_pose.shape[0], np.random.default_rng(seed))


@pytest.fixture(scope="module")
def cfg():
    from ga_ddpg_amd.experiments.config import load_cfg
    return load_cfg("ddpg_td3_aux.yaml")


def _host_goals(cfg, poses, flags, idx, end):
    """the host path's own answer on these rows: BaseMemory.onpolicy_goals of a buffer whose slots 2k, 2k + 1 hold row k's own
    pose and the pose its episode ended in (a row index may repeat with another end, so the rows get slots of their own)"""
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    idx, end = np.asarray(idx), np.asarray(end)
    n = len(idx)
    mem = BaseMemory(2 * n, cfg, name="online", point_dtype=np.float32)
    mem.state_pose[0::2], mem.state_pose[1::2] = poses[idx], poses[end]
    mem.expert_flags[0::2] = np.asarray(flags)[idx]
    mem.episode_map[0::2] = 2 * np.arange(n) + 1
    mask, goal, _ = mem.onpolicy_goals(2 * np.arange(n))
    np.testing.assert_array_equal(mask, np.asarray(flags)[idx] == 0.0)
    return np.asarray(goal, dtype=np.float64)


def _sentinel(rows):
    return (7000.0 + np.arange(rows * 7, dtype=np.float64).reshape(rows, 7) * 0.25 + 0.125).astype(np.float32)


def _launch(srcs, row_start, idx, end, B, shift=0, extra_rows=3):
    """one gad_replay_relabel_goals call.  srcs[s]: (poses (cap, 4, 4) float32, flags (cap) float32), or None = all NULL.
    -> (out_goal rows [0, B + extra_rows), the sentinel it was prefilled with); inputs are checked untouched"""
    hip = _hip()
    bufs = [None if s is None else (Buf(s[0].reshape(-1, 16), shift=shift), Buf(s[1])) for s in srcs]
    bi, be = Buf(np.asarray(idx, dtype=np.int64)), Buf(np.asarray(end, dtype=np.int64))
    fill = _sentinel(B + extra_rows)
    out = Buf(fill)
    a = hip.ReplayRelabelArgs()
    a.B, a.n_src = B, len(srcs)
    for s, r in enumerate(row_start):
        a.row_start[s] = int(r)
    for s, b in enumerate(bufs):
        if b is not None:
            a.src[s].state_pose, a.src[s].expert_flags = b[0].ptr, b[1].ptr
    a.idx, a.end, a.out_goal = bi.ptr, be.ptr, out.ptr
    hip.call_struct("gad_replay_relabel_goals", a)
    got = out.get("out_goal")                                           # (Buf.get checks the guard bytes too)
    for s, b in enumerate(bufs):
        if b is not None:
            _same("source %d poses untouched" % s, b[0].get(), srcs[s][0].reshape(-1, 16))
            _same("source %d flags untouched" % s, b[1].get(), srcs[s][1])
    return got, fill


def _kernel_case(seed):
    """the seeded inputs of the kernel test: per source ~96 rigid poses and flags; rows with idx == end and expert rows present"""
    rng = np.random.default_rng(seed)
    srcs, idx, end = [], [], []
    for s in range(4):
        n = ROW_START[s + 1] - ROW_START[s]
        flags = rng.choice(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 2.0, -1.0], np.float32), CAP)
        srcs.append((_rigid(CAP, rng), flags))
        i, e = rng.integers(0, CAP, n), rng.integers(0, CAP, n)
        if n >= 6:
            on, ex = np.flatnonzero(flags == 0), np.flatnonzero(flags != 0)
            i[0], i[1], i[2], i[-1] = on[0], ex[0], on[1], on[2]         # first / last row of the source: on-policy
            e[2] = i[2]                                                 # idx == end: the identity goal
            e[-1] = i[-1]
            i[3], i[4] = 0, CAP - 1                                     # the first and the last pose of the source
            e[5] = CAP - 1
        idx.append(i)
        end.append(e)
    return srcs, np.concatenate(idx).astype(np.int64), np.concatenate(end).astype(np.int64)


# ----------------------------------------------------------------------------- 1, 2: the kernel
@pytest.mark.parametrize("shift", (0, 8))                                # 8: poses two floats off 16-byte alignment (scalar loads)
def test_relabel_kernel_against_float64_closed_form(cfg, shift):
    srcs, idx, end = _kernel_case(9100)
    B = ROW_START[-1]
    launch_srcs = [srcs[0], None, srcs[2], None]                         # source 1: rows but NULL poses; source 3: no rows
    got, fill = _launch(launch_srcs, ROW_START, idx, end, B, shift=shift)
    relabelled = np.zeros(B + 3, dtype=bool)
    dev, host, ref = [], [], []
    for s in (0, 2):
        lo, hi = ROW_START[s], ROW_START[s + 1]
        poses, flags = srcs[s]
        on = flags[idx[lo:hi]] == 0.0
        assert on.any() and (~on).any() and (idx[lo:hi][on] == end[lo:hi][on]).any()
        relabelled[lo:hi] = on
        dev.append(got[lo:hi][on])
        ref.append(_goals64(poses, idx[lo:hi][on], end[lo:hi][on]))
        host.append(_host_goals(cfg, poses, flags, idx[lo:hi], end[lo:hi])[on])
        same = idx[lo:hi][on] == end[lo:hi][on]
        assert np.abs(dev[-1][same] - np.array([1, 0, 0, 0, 0, 0, 0.0])).max() <= 2e-6      # idx == end: the identity
    # expert rows, every row of the source without poses and the rows past B: bit-identical to the prefill
    _same("rows the kernel must not write", got[~relabelled], fill[~relabelled])
    assert relabelled[:B].sum() >= 20 and not (got[relabelled] == fill[relabelled]).all(axis=1).any()
    _gate("kernel B = %d shift %d" % (B, shift), np.concatenate(dev), np.concatenate(host), np.concatenate(ref))
    # B = 1: one source, one on-policy row
    poses, flags = srcs[0]
    i = np.flatnonzero(flags == 0)[3:4]
    e = np.array([CAP - 1])
    got1, fill1 = _launch([srcs[0]], (0, 1), i, e, 1, shift=shift)
    _same("B = 1: rows past B", got1[1:], fill1[1:])
    _gate("kernel B = 1", got1[:1], _host_goals(cfg, poses, flags, i, e), _goals64(poses, i, e))
    # ... and one expert row: nothing is written
    x = np.flatnonzero(flags != 0)[:1]
    got1, fill1 = _launch([srcs[0]], (0, 1), x, e, 1, shift=shift)
    _same("B = 1, expert row", got1, fill1)


# ----------------------------------------------------------------------------- 3: the four branches
def _pairs(rel, A):
    """poses [A_0, E_0, A_1, E_1, ...] with E_k = A_k . rel_k formed in float64 and stored as float32"""
    P = np.zeros((2 * len(rel), 4, 4), dtype=np.float32)
    for k, (R, t) in enumerate(rel):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, t
        P[2 * k], P[2 * k + 1] = A[k], (A[k].astype(np.float64) @ M)
    return P


def test_relabel_kernel_takes_each_quaternion_branch(cfg):
    rng = np.random.default_rng(9200)
    axes = np.eye(3)
    rel, want_branch, A = [], [], []
    for on_identity in (False, True):                                   # seen from random poses, and from pure translations
        for k in range(3):                                              # 3.0 rad about x, y, z: the largest component is x, y, z
            rel.append((_axis_angle(axes[k], 3.0), rng.normal(size=3)))
            want_branch.append(k + 1)
        rel.append((_axis_angle(rng.normal(size=3), 0.1), rng.normal(size=3)))         # a small rotation: the trace branch
        want_branch.append(0)
        for k in range(3):                                              # exactly pi about each axis (w = 0: compared sign-free)
            rel.append((np.diag([1.0 if j == k else -1.0 for j in range(3)]), rng.normal(size=3)))
            want_branch.append(k + 1)
        poses = _rigid(7, rng)
        if on_identity:
            poses[:, :3, :3] = np.eye(3)
        A.extend(poses)
    P = _pairs(rel, A)
    n = len(rel)
    idx, end = 2 * np.arange(n), 2 * np.arange(n) + 1
    flags = np.zeros(2 * n, dtype=np.float32)
    got, _ = _launch([(P, flags)], (0, n), idx, end, n)
    dev, ref = got[:n], _goals64(P, idx, end)
    assert [int(np.argmax(np.abs(r[:4]))) for r in ref] == want_branch
    assert (ref[:, 0] < 0.08).sum() == 12 and (ref[:, 0] < 1e-3).sum() == 6          # w ~ 0.07 at 3.0 rad, ~ 0 at pi
    host = _host_goals(cfg, P, flags, idx, end)
    for k in range(n):
        _gate("branch case %d (largest component %d)" % (k, want_branch[k]), dev[k:k + 1], host[k:k + 1], ref[k:k + 1])
        R64 = (np.linalg.inv(P[idx[k]].astype(np.float64)) @ P[end[k]].astype(np.float64))[:3, :3]
        assert np.abs(_rot64(dev[k, :4]) - R64).max() <= 5e-6, k


# ----------------------------------------------------------------------------- 4: non-finite input
def test_relabel_kernel_writes_the_identity_for_a_nan_pose(cfg):
    rng = np.random.default_rng(9300)
    P = _rigid(8, rng)
    P[3, 1, 2] = np.nan                                                 # one NaN entry in a rotation
    flags = np.zeros(8, dtype=np.float32)
    idx = np.array([0, 2, 3, 4, 5, 6])
    end = np.array([1, 7, 7, 3, 7, 0])                                  # row 2 starts at the NaN pose, row 3 ends in it
    got, _ = _launch([(P, flags)], (0, 6), idx, end, 6)
    for b in (2, 3):
        _same("NaN pose, row %d: identity quaternion" % b, got[b, :4], np.array([1, 0, 0, 0], np.float32))
    ok = np.array([0, 1, 4, 5])
    _gate("neighbours of the NaN rows", got[ok], _host_goals(cfg, P, flags, idx[ok], end[ok]), _goals64(P, idx[ok], end[ok]))


# ----------------------------------------------------------------------------- 5: DeviceReplay(relabel="device")
def _raise_onpolicy_goals(monkeypatch):
    from ga_ddpg_amd.core.replay_memory import BaseMemory

    def boom(self, batch_idx):
        raise AssertionError("BaseMemory.onpolicy_goals called on the device-relabel path")
    monkeypatch.setattr(BaseMemory, "onpolicy_goals", boom)


def _count_launches(monkeypatch):
    from ga_ddpg_amd.core import device_replay
    calls, inner = [], device_replay._launch_relabel

    def counting(*a, **kw):
        calls.append(a[0])
        return inner(*a, **kw)
    monkeypatch.setattr(device_replay, "_launch_relabel", counting)
    return calls


def _check_against_host(what, goal, mem, idx, host_goal, host_on):
    """device goals `goal` (B, 7) of buffer rows idx: bit-equal on expert rows, within the gate on the relabelled ones"""
    idx = np.asarray(idx)
    on = mem.expert_flags[idx] == 0.0
    host_goal = np.asarray(host_goal, dtype=np.float32)
    _same(what + ": expert rows", goal[~on], host_goal[~on])
    if on.any():
        end = np.asarray(mem.episode_map[idx], dtype=np.int64)
        _gate(what, goal[on], host_on[on], _goals64(mem.state_pose, idx[on], end[on]))


def test_device_replay_forms_the_goals_on_the_device(monkeypatch):
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    from ga_ddpg_amd.core.prefetch import PrefetchSampler
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.runtime import BATCH_KEYS
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    mem = BaseMemory(700, cfg, point_dtype=np.float32)                   # the buffer of test_device_replay_relabels_onpolicy_goals_...
    fill_synthetic_buffer(mem, 700, seed=5)
    mem.name, mem.self_supervision = "online", True
    _rigid_poses(mem, 2)
    idx = mem.draw_indices(24, np.random.default_rng(1))
    assert (mem.expert_flags[idx] == 0).any() and (mem.expert_flags[idx] != 0).any()     # both kinds of rows are in the batch
    host = mem.sample(24, batch_idx=idx)                                # (before onpolicy_goals is made to raise)
    host_on = mem.onpolicy_goals(idx)[1]
    assert np.abs(host["goal_batch"] - mem.goal[idx]).max() > 1e-3       # the relabelling changed some goals
    with pytest.raises(ValueError):
        DeviceReplay(mem, relabel="sideways")
    assert DeviceReplay(mem).state_pose is None                         # the poses are mirrored in device mode only
    _raise_onpolicy_goals(monkeypatch)
    calls = _count_launches(monkeypatch)
    dmem = DeviceReplay(mem, relabel="device")
    assert tuple(dmem.state_pose.shape) == (700, 16)
    dev = dmem.sample(24, batch_idx=idx)
    assert len(calls) == 1
    for k in BATCH_KEYS:
        if k != "goal_batch":
            np.testing.assert_array_equal(dev[k].cpu().numpy(), np.asarray(host[k], dtype=np.float32).reshape(dev[k].shape), err_msg=k)
    goal = dev["goal_batch"].cpu().numpy()
    _check_against_host("DeviceReplay.sample", goal, mem, idx, host["goal_batch"], host_on)
    rt = agent.runtime(24, host["point_state_batch"].shape[2])
    lazy = dmem.sample_lazy(24, batch_idx=idx)
    assert lazy["relabel_mode"] == "device"
    rt.upload(lazy)
    torch.cuda.synchronize()
    assert len(calls) == 2
    _same("lazy handle = sample()", rt.dbuf["goal_batch"].cpu().numpy(), goal)
    for k in BATCH_KEYS:
        if k != "goal_batch":
            np.testing.assert_array_equal(rt.dbuf[k].cpu().numpy(), np.asarray(host[k], dtype=np.float32).reshape(rt.dbuf[k].shape),
                                          err_msg="lazy " + k)
    with PrefetchSampler(dmem, 24, depth=2, rng=np.random.default_rng(1)) as s:         # the same first draw as `idx`
        pre = s.next()
        np.testing.assert_array_equal(pre["batch_idx"], np.uint8(idx))
        rt.upload(pre)
        torch.cuda.synchronize()
    _same("prefetched handle = sample()", rt.dbuf["goal_batch"].cpu().numpy(), goal)
    # a buffer that does not relabel: stored goals bit for bit, and no launch of the new entry point
    mem.self_supervision = False
    n = len(calls)
    plain = dmem.sample(24, batch_idx=idx)
    rt.upload(dmem.sample_lazy(24, batch_idx=idx))
    torch.cuda.synchronize()
    assert len(calls) == n
    _same("no relabelling: sample()", plain["goal_batch"].cpu().numpy(), mem.goal[idx])
    _same("no relabelling: lazy", rt.dbuf["goal_batch"].cpu().numpy(), mem.goal[idx])


# ----------------------------------------------------------------------------- 6: MixedDeviceReplay
def _two_buffers(cfg, online_cap=200, online_fill=170):
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    expert = BaseMemory(400, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(expert, 400, seed=31)
    online = BaseMemory(online_cap, cfg, name="online", point_dtype=np.float32)
    fill_synthetic_buffer(online, online_fill, seed=32)
    online.self_supervision = True
    _rigid_poses(online, 2)
    return expert, online


def _mixed_cases(expert, online):
    """(sizes, per-part indices): on-policy and expert rows of the online buffer in turn (tests/test_gpu_mixed_replay.py)"""
    hi = online.upper_idx()
    kinds = [np.flatnonzero(online.expert_flags[:hi] == 0), np.flatnonzero(online.expert_flags[:hi] != 0)]
    for sizes in ((5, 3), (8, 0), (0, 8)):
        idx = [expert.draw_indices(sizes[0], np.random.default_rng(40)),
               np.array([kinds[j % 2][(7 * j) % len(kinds[j % 2])] for j in range(sizes[1])], dtype=np.int64)]
        yield sizes, idx


@pytest.mark.parametrize("modes", (("host", "device"), ("device", "device"), ("host", "host")))
def test_mixed_device_replay_relabels_per_part(modes, monkeypatch):
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.device_replay import DeviceReplay, MixedDeviceReplay
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    from ga_ddpg_amd.runtime import BATCH_KEYS
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    expert, online = _two_buffers(cfg)
    cases = [(sizes, idx, sample_mixed((expert, online), sizes, batch_idx=idx), online.onpolicy_goals(idx[1])[1])
             for sizes, idx in _mixed_cases(expert, online)]           # (the host's answers, before onpolicy_goals is made to raise)
    if modes[1] == "device":
        _raise_onpolicy_goals(monkeypatch)
    calls = _count_launches(monkeypatch)
    d0, d1 = DeviceReplay(expert, relabel=modes[0]), DeviceReplay(online, relabel=modes[1])
    rt = agent.runtime(8, expert.point_state.shape[2])
    for sizes, idx, host, host_on in cases:
        mixed = MixedDeviceReplay([(d0, sizes[0]), (d1, sizes[1])])
        n = len(calls)
        dev = mixed.sample(batch_idx=idx)
        lazy = mixed.sample_lazy(batch_idx=idx)
        assert lazy["relabel_mode"] == modes
        rt.upload(lazy)
        torch.cuda.synchronize()
        assert len(calls) - n == (2 if modes[1] == "device" and sizes[1] else 0), (sizes, modes)
        for k in BATCH_KEYS:
            for what, got in (("eager", dev[k].cpu().numpy()), ("lazy", rt.dbuf[k].cpu().numpy())):
                want = np.asarray(host[k], dtype=np.float32).reshape(got.shape)
                if k != "goal_batch" or modes[1] == "host":             # host mode: bit-equal to today's
                    np.testing.assert_array_equal(got, want, err_msg="%s %s %s" % (what, sizes, k))
                    continue
                _same("%s %s: expert part" % (what, sizes), got[:sizes[0]], want[:sizes[0]])
                if sizes[1]:
                    _check_against_host("mixed %s %s %s" % (modes, what, sizes), got[sizes[0]:], online, idx[1], want[sizes[0]:], host_on)
        _same("lazy = eager %s" % (sizes,), rt.dbuf["goal_batch"].cpu().numpy(), dev["goal_batch"].cpu().numpy())


# ----------------------------------------------------------------------------- 7: writes
def _rollout(mem, n, tag, poses):
    shape = mem.point_state.shape[1:]
    return [{"point_state": np.full(shape, float(tag + t), dtype=np.float32), "action": np.full(6, 0.001 * (tag + t), np.float32),
             "expert_action": np.full(6, -0.001 * (tag + t), np.float32), "goal": np.full(7, 0.01 * t, np.float32),
             "reward": float(t == n - 1), "terminal": float(t == n - 1), "timestep": float(t), "expert_flags": float(t == 1),
             "perturb_flags": 0.0, "state_pose": poses[t], "target_name": "box"} for t in range(n)]


def test_device_relabel_follows_writes(cfg):
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    expert, online = _two_buffers(cfg, online_cap=200, online_fill=170)
    online.RL = True
    dmem = DeviceReplay(online, relabel="device")
    new = _rigid(6, np.random.default_rng(77))
    start = online.cur_idx
    online.add_episode(_rollout(online, 6, 3000, new))
    slots = np.arange(start, start + 6)
    np.testing.assert_array_equal(online.state_pose[slots], new)
    assert (online.episode_map[slots] == start + 5).all()
    before = dmem.uploaded_cloud_rows
    assert dmem.sync_writes() == 6 and dmem.uploaded_cloud_rows - before == 6          # the pushed slots' clouds only
    _same("mirrored poses", dmem.state_pose[:online.upper_idx()].cpu().numpy(), online.state_pose[:online.upper_idx()].reshape(-1, 16))
    host_on = online.onpolicy_goals(slots)[1]
    host = online.sample(6, batch_idx=slots)
    got = dmem.sample(6, batch_idx=slots)["goal_batch"].cpu().numpy()
    assert (online.expert_flags[slots] != 0).sum() == 1
    _check_against_host("after add_episode + sync_writes", got, online, slots, host["goal_batch"], host_on)
    # direct writes announced by mark_rewritten(): the full refresh carries the poses too
    rows = np.arange(40, 52)
    rows = rows[online.expert_flags[rows] == 0][:4]
    ends = np.asarray(online.episode_map[rows], dtype=np.int64)
    old = dmem.sample(len(rows), batch_idx=rows)["goal_batch"].cpu().numpy()
    online.state_pose[np.r_[rows, ends]] = _rigid(2 * len(rows), np.random.default_rng(78))
    online.mark_rewritten()
    before = dmem.uploaded_cloud_rows
    assert dmem.sync_writes() == online.upper_idx() == dmem.uploaded_cloud_rows - before
    host_on = online.onpolicy_goals(rows)[1]
    host = online.sample(len(rows), batch_idx=rows)
    got = dmem.sample(len(rows), batch_idx=rows)["goal_batch"].cpu().numpy()
    assert np.abs(got - old).max() > 1e-3
    _check_against_host("after mark_rewritten + sync_writes", got, online, rows, host["goal_batch"], host_on)


# ----------------------------------------------------------------------------- 8: one DDPG update
def test_update_on_device_relabelled_goals_equals_host_relabelled():
    """B = 24, the same indices and the same injected noise: the 11-key logs of an update fed from a device-mode handle agree with
    those of one fed from a host-mode handle to 1e-4 relative (+ 1e-6: tests/smoke_step.py's bar).  Both updates run in the
    deterministic mode, so the goals' float32 rounding is the only difference between them (in the default mode the atomics'
    run-to-run noise alone is allowed 2e-3 by tests/test_gpu_modules.py::test_device_replay_matches_host_sampling)."""
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    from oracle.detfill import fill_module_
    prev = hip.get_option("deterministic")
    hip.set_option("deterministic", 1)
    try:
        agents = []
        for _ in range(2):
            a, cfg = make_agent("ddpg_td3_aux.yaml")
            for name in ("policy", "policy_target", "critic", "critic_target", "state_feature_extractor"):
                fill_module_(getattr(a, name), name, 7)
            agents.append(a)
        mem = BaseMemory(700, cfg, point_dtype=np.float32)
        fill_synthetic_buffer(mem, 700, seed=5)
        mem.name, mem.self_supervision = "online", True
        _rigid_poses(mem, 2)
        idx = mem.draw_indices(24, np.random.default_rng(1))
        flags, ret, per = mem.expert_flags[idx], mem.returns[idx], mem.perturb_flags[idx]
        assert (flags == 0).any() and (flags >= 1).any() and (ret > 0).any() and (per < 1).any()      # the masked means are defined
        u = np.random.default_rng(5).random((24, 6)).astype(np.float32)
        r_host = agents[0].update_parameters(DeviceReplay(mem).sample_lazy(24, batch_idx=idx), agents[0].update_step, 0, noise_u=u)
        r_dev = agents[1].update_parameters(DeviceReplay(mem, relabel="device").sample_lazy(24, batch_idx=idx),
                                            agents[1].update_step, 0, noise_u=u)
        torch.cuda.synchronize()
    finally:
        hip.set_option("deterministic", prev)
    assert set(r_dev) == set(r_host) and len(r_host) == 11
    for k in sorted(r_host):
        print("%-28s host-mode %.9g device-mode %.9g" % (k, r_host[k], r_dev[k]))
    for k in r_host:
        assert_close(r_dev[k], r_host[k], 1e-4, 1e-6, k)


# ----------------------------------------------------------------------------- 9: train_off_policy
TRAIN_SEED = 0


def test_train_off_policy_with_device_relabel(monkeypatch):
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core import train_test_offline as tto
    from ga_ddpg_amd.core.replay_memory import sample_mixed
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    config = cfg.RL_TRAIN
    assert config.onpolicy and config.online_buffer_ratio == 1.0      # the shipped configuration
    config.batch_size, config.updates_per_step, config.max_epoch, config.save_epoch = 8, 2, 1000, []
    expert, online = _two_buffers(cfg)
    rng = np.random.default_rng(TRAIN_SEED)
    for _ in range(6):                                                 # (a property of the seeded buffers and TRAIN_SEED)
        b = sample_mixed((expert, online), (8, 8), rng=rng)
        assert (b["expert_flag_batch"] >= 1).any() and (b["return_batch"] > 0).any() and (b["perturb_flag_batch"] < 1).any()
    _raise_onpolicy_goals(monkeypatch)
    calls = _count_launches(monkeypatch)
    logs = []
    losses, epochs = tto.train_off_policy(agent, expert, config, None, save_model=False, max_epochs=3, log=logs.append,
                                          device_replay=True, rng=np.random.default_rng(TRAIN_SEED), online_memory=online,
                                          device_relabel=True)
    assert epochs == 3 and len(calls) == 6 and all(b == 16 for b in calls)
    assert all(np.isfinite(list(h)).all() for h in losses.values())
    assert len(losses["critic_loss"]) == 7                              # deque([0]) + 6 updates
    assert any("mirrored in HBM" in l and "hindsight goals formed on the device" in l for l in logs)
    assert tto.device_mirror(online, "device").relabel == "device" and tto.device_mirror(online).relabel == "host"
    assert tto.device_mirror(expert, "device") is tto.device_mirror(expert)              # an expert buffer never relabels
