"""Step rate of train_off_policy on the shipped two-buffer batch (ddpg_td3_aux: 128 expert + 128 online rows), synthetic buffers,
the synchronous loop, one GPU:
  (a) single-buffer device replay at B = 256   -- the existing path, the yardstick; its own run-to-run spread
  (b) the mixed device path                    -- MixedDeviceReplay, one gad_replay_gather_multi launch per minibatch
  (c) the host path                            -- replay_memory.sample_mixed + upload
The three loops alternate (a b c a b c ...) inside one process on one agent (all three train on 256 rows: one runtime).
    python tools/diag_mixed_replay.py [--rounds 3] [--epochs 6] [--out profiles/mixed_replay.txt] [--commit ID]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/diag_mixed_replay.py --gathers 300     (the two gather kernels alone)
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=6, help="timed epochs of 50 updates per loop and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_replay.txt"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--gathers", type=int, default=0, help="only run this many single and mixed gathers (for a kernel trace)")
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

    if args.gathers:
        single, mixed = device_mirror(expert), mixed_device_mirror(expert, online, 128, 128)
        rt = agent.runtime(256, expert.point_state.shape[2])
        rng = np.random.default_rng(0)
        for _ in range(args.gathers):
            rt.upload(single.sample_lazy(256, rng=rng))
            rt.upload(mixed.sample_lazy(rng=rng))
        torch.cuda.synchronize()
        print("%d gad_replay_gather + %d gad_replay_gather_multi launches at B = 256" % (args.gathers, args.gathers))
        return

    def loop(which, epochs):
        c.batch_size = 256 if which == "a" else 128
        kw = dict(max_epochs=epochs, rng=np.random.default_rng(3))
        if which == "a":
            train_off_policy(agent, expert, c, device_replay=True, **kw)
        else:
            train_off_policy(agent, expert, c, device_replay=(which == "b"), online_memory=online, **kw)

    names = {"a": "single-buffer device replay, B = 256", "b": "mixed device replay, 128 + 128", "c": "host sample_mixed, 128 + 128"}
    for which in "abc":                                                # warm-up: mirrors, runtime, plans, pinned buffers
        loop(which, 1)
    rates = {k: [] for k in "abc"}
    for _ in range(args.rounds):
        for which in "abc":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(which, args.epochs)
            torch.cuda.synchronize()
            rates[which].append(args.epochs * c.updates_per_step / (time.perf_counter() - t0))
    lines = ["mixed expert + online replay: steps/s of train_off_policy (synchronous loop, lookahead on), ddpg_td3_aux, 256 rows",
             "commit: %s" % (args.commit or _commit()),
             "command: python tools/diag_mixed_replay.py --rounds %d --epochs %d" % (args.rounds, args.epochs),
             "device: %s; %d updates per timed window; loops alternate a b c per round" % (
                 torch.cuda.get_device_name(0), args.epochs * c.updates_per_step)]
    for k in "abc":
        r = rates[k]
        lines.append("(%s) %-40s %s   median %.1f  min %.1f  max %.1f steps/s" % (
            k, names[k], " ".join("%.1f" % x for x in r), float(np.median(r)), min(r), max(r)))
    a, b = rates["a"], rates["b"]
    inside = min(a) <= float(np.median(b)) <= max(a)
    lines.append("expectation: (b) within (a)'s own spread (the same step + one gather launch of the same bytes): %s -- median (b) / "
                 "median (a) = %.3f, (a) spread %.1f %%" % ("yes" if inside else "NO", float(np.median(b)) / float(np.median(a)),
                                                            100.0 * (max(a) - min(a)) / float(np.median(a))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
