"""Step rate of train_off_policy on the shipped two-buffer batch (ddpg_td3_aux: 128 expert + 128 online rows), synthetic buffers,
the synchronous loop, one GPU:
  (a) single-buffer device replay at B = 256   -- the existing path, the yardstick; its own run-to-run spread
  (b) the mixed device path                    -- MixedDeviceReplay, one gad_replay_gather_multi launch per minibatch
  (c) the host path                            -- replay_memory.sample_mixed + upload
  (d) (b) with a self-supervised online buffer -- its hindsight goals formed on the host (BaseMemory.onpolicy_goals per draw)
  (e) (d) with device_relabel=True             -- the goals formed by one gad_replay_relabel_goals launch behind the gather
The five loops alternate (a b c d e a b ...) inside one process on one agent (all train on 256 rows: one runtime).  (d) and (e)
draw from a copy of the online buffer that shares its arrays but relabels (self_supervision, rigid poses); the accuracy of the
device goals against a float64 closed form, with the host's goals as the yardstick, is measured on 640 of its rows.
    python tools/diag_mixed_replay.py [--rounds 3] [--epochs 6] [--out profiles/device_relabel.txt] [--commit ID]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diag_mixed_replay.py --gathers 300     (the gather and relabel kernels alone)
(profiles/mixed_replay.txt is the output of the three-leg version of this tool.)
"""
import argparse
import copy
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def _rot(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _goal64(A, E):
    """[quaternion (w >= 0) | translation] of inv(A) @ E in float64: the closed form that divides by the largest component"""
    M = np.linalg.inv(np.asarray(A, dtype=np.float64)) @ np.asarray(E, dtype=np.float64)
    R = M[:3, :3]
    c = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2],
                  1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(c))
    v = [np.array([c[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]),
         np.array([R[2, 1] - R[1, 2], c[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]]),
         np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], c[2], R[1, 2] + R[2, 1]]),
         np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], c[3]])][k]
    q = v / np.linalg.norm(v)
    return np.r_[-q if q[0] < 0 else q, M[:3, 3]]


def _err(got, ref):
    """max |got - ref| over quaternion and translation; rows whose float64 w < 1e-3 compare the quaternion up to its sign"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    dq = np.abs(got[:, :4] - ref[:, :4]).max(axis=1)
    free = ref[:, 0] < 1e-3
    dq[free] = np.minimum(dq, np.abs(got[:, :4] + ref[:, :4]).max(axis=1))[free]
    return float(max(dq.max(), np.abs(got[:, 4:] - ref[:, 4:]).max()))


def relabelling_copy(online, seed=7):
    """a buffer that shares `online`'s arrays but forms hindsight goals: self_supervision on, rigid poses of its own (uniform
    rotations, unit-normal translations).  Made before any mirror hangs on `online`, so each buffer gets mirrors of its own."""
    mem = copy.copy(online)
    mem.self_supervision = True
    rng = np.random.default_rng(seed)
    mem.state_pose = np.zeros_like(online.state_pose)
    for i in range(len(mem.state_pose)):
        mem.state_pose[i] = np.eye(4)
        mem.state_pose[i][:3, :3] = _rot(rng.normal(size=4))
        mem.state_pose[i][:3, 3] = rng.normal(size=3)
    return mem


def accuracy_lines(mem, rows=640):
    """device goals and host goals of `rows` drawn transitions of `mem` against float64"""
    from ga_ddpg_amd.core.device_replay import DeviceReplay
    idx = mem.draw_indices(rows, np.random.default_rng(11))
    mask, host, _ = mem.onpolicy_goals(idx)
    mask = np.asarray(mask).reshape(-1)
    dev = DeviceReplay(mem, relabel="device").sample(rows, batch_idx=idx)["goal_batch"].cpu().numpy()
    end = np.asarray(mem.episode_map[idx], dtype=np.int64)
    ref = np.array([_goal64(mem.state_pose[i], mem.state_pose[e]) for i, e in zip(idx[mask], end[mask])])
    e_dev, e_host = _err(dev[mask], ref), _err(np.asarray(host)[mask], ref)
    same = bool((dev[~mask] == np.asarray(mem.goal[idx], dtype=np.float32)[~mask]).all())
    q = dev[mask][:, :4].astype(np.float64)
    return ["accuracy on %d drawn rows of the relabelling online buffer, %d of them on-policy (relabelled), against the float64 closed form:"
            % (rows, int(mask.sum())),
            "  err = max |x - f64| over quaternion and translation; rows with float64 w < 1e-3 (%d) compare the quaternion up to sign"
            % int((ref[:, 0] < 1e-3).sum()),
            "  err(device, gad_replay_relabel_goals) %.3g   err(host, BaseMemory.onpolicy_goals) %.3g   gate max(3 x host, 2e-6) = %.3g: %s"
            % (e_dev, e_host, max(3 * e_host, 2e-6), "met" if e_dev <= max(3 * e_host, 2e-6) else "NOT MET"),
            "  min w %.3g   max | |q| - 1 | %.3g   expert rows bit-equal to the stored goals: %s"
            % (float(q[:, 0].min()), float(np.abs(np.linalg.norm(q, axis=1) - 1).max()), "yes" if same else "NO")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=6, help="timed epochs of 50 updates per loop and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_relabel.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--gathers", type=int, default=0, help="only run this many single, mixed and mixed + device-relabel gathers "
                                                           "(for a kernel trace)")
    args = ap.parse_args()
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.replay_memory import BaseMemory
    from ga_ddpg_amd.core.train_test_offline import device_mirror, mixed_device_mirror, train_off_policy
    from ga_ddpg_amd.synth_data import fill_synthetic_buffer
    if not torch.cuda.is_available():
        raise SystemExit("diag_mixed_replay measures on a GPU; none found")
    agent, cfg = make_agent("ddpg_td3_aux.yaml")
    c = cfg.RL_TRAIN
    c.updates_per_step, c.max_epoch, c.save_epoch = 50, 10 ** 9, []
    assert c.onpolicy and c.online_buffer_ratio == 1.0
    expert = BaseMemory(20000, cfg, point_dtype=np.float32)
    fill_synthetic_buffer(expert, 20000, seed=1)
    online = BaseMemory(10000, cfg, name="online", point_dtype=np.float32)
    fill_synthetic_buffer(online, 10000, seed=2)
    online_r = relabelling_copy(online)

    if args.gathers:
        single, mixed = device_mirror(expert), mixed_device_mirror(expert, online, 128, 128)
        mixed_e = mixed_device_mirror(expert, online_r, 128, 128, "device")
        rt = agent.runtime(256, expert.point_state.shape[2])
        rng = np.random.default_rng(0)
        for _ in range(args.gathers):
            rt.upload(single.sample_lazy(256, rng=rng))
            rt.upload(mixed.sample_lazy(rng=rng))
            rt.upload(mixed_e.sample_lazy(rng=rng))
        torch.cuda.synchronize()
        print("%d gad_replay_gather + %d gad_replay_gather_multi + %d gad_replay_relabel_goals launches at B = 256"
              % (args.gathers, 2 * args.gathers, args.gathers))
        return

    def loop(which, epochs):
        c.batch_size = 256 if which == "a" else 128
        kw = dict(max_epochs=epochs, rng=np.random.default_rng(3))
        if which == "a":
            train_off_policy(agent, expert, c, device_replay=True, **kw)
        elif which in "bc":
            train_off_policy(agent, expert, c, device_replay=(which == "b"), online_memory=online, **kw)
        else:
            train_off_policy(agent, expert, c, device_replay=True, online_memory=online_r, device_relabel=(which == "e"), **kw)

    names = {"a": "single-buffer device replay, B = 256", "b": "mixed device replay, 128 + 128", "c": "host sample_mixed, 128 + 128",
             "d": "mixed, online relabels: goals on host", "e": "mixed, online relabels: goals on device"}
    legs = "abcde"
    for which in legs:                                                 # warm-up: mirrors, runtime, plans, pinned buffers
        loop(which, 1)
    rates = {k: [] for k in legs}
    for _ in range(args.rounds):
        for which in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(which, args.epochs)
            torch.cuda.synchronize()
            rates[which].append(args.epochs * c.updates_per_step / (time.perf_counter() - t0))
    lines = ["hindsight goals on the host vs on the device: steps/s of train_off_policy (synchronous loop, lookahead on), ddpg_td3_aux, "
             "256 rows",
             "commit: %s" % (args.commit or _commit()),
             "command: python tools/diag_mixed_replay.py --rounds %d --epochs %d" % (args.rounds, args.epochs),
             "device: %s; %d updates per timed window; loops alternate a b c d e per round" % (
                 torch.cuda.get_device_name(0), args.epochs * c.updates_per_step)]
    for k in legs:
        r = rates[k]
        lines.append("(%s) %-40s %s   median %.1f  min %.1f  max %.1f steps/s" % (
            k, names[k], " ".join("%.1f" % x for x in r), float(np.median(r)), min(r), max(r)))
    a, b = rates["a"], rates["b"]
    inside = min(a) <= float(np.median(b)) <= max(a)
    lines.append("expectation: (b) within (a)'s own spread (the same step + one gather launch of the same bytes): %s -- median (b) / "
                 "median (a) = %.3f, (a) spread %.1f %%" % ("yes" if inside else "NO", float(np.median(b)) / float(np.median(a)),
                                                            100.0 * (max(a) - min(a)) / float(np.median(a))))
    d, e = rates["d"], rates["e"]
    md, me, mb = float(np.median(d)), float(np.median(e)), float(np.median(b))
    lines.append("expectation: (e) beats (d) by more than both legs' run-to-run spread (min (e) > max (d)): %s -- median (e) / median (d) "
                 "= %.3f, (d) spread %.1f %%, (e) spread %.1f %%" % ("yes" if min(e) > max(d) else "NO", me / md,
                                                                   100.0 * (max(d) - min(d)) / md, 100.0 * (max(e) - min(e)) / me))
    lines.append("reported, not gated: median (e) / median (b) = %.3f (the same step + one relabel launch of B lanes; (b) spread %.1f %%)"
                 % (me / mb, 100.0 * (max(b) - min(b)) / mb))
    lines += accuracy_lines(online_r)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
