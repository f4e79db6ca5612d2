"""Times gad_fps_tiled (one launch per pick, include/gaddpg.h section A) at B = 1, M = 1024 for clouds of 8192 .. 262144 points and
four slice sizes, i.e. four values of `groups`.  Recorded, not gated (the correctness gates are tests/test_gpu_fps_tiled.py);
the library's rule for groups = 0 (FPS_TILED_SLICE in csrc/fps.hip) is taken from this table.

    python tools/diag_fps_tiled.py [--out profiles/fps_tiled.txt] [--rounds 5]

Per (N, slice): the device time of one call (events around it, median over the rounds) divided by the M + 1 launches = time per
round; the bytes a round moves (N x 20: 12 of coordinates, 4 + 4 of the running minimum, the store only where it shrank) against
the HBM peak; the host time to enqueue the call's launches (the stream drained first, the clock stopped when the call returns).
At N = 8192 the one-workgroup LDS kernel (gad_furthest_point_sampling) runs beside it: the only shape both accept here.
Every N runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the run."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (8192, 32768, 131072, 262144)
SLICES = (256, 1024, 4096, 16384)
M = 1024
HBM_PEAK = 8.0e12                        # bytes / s (MI355X data sheet)
CHILD_LIMIT = 120                        # seconds per N


def child(N, rounds):
    import numpy as np
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.synth_data import box_surface_cloud
    if not torch.cuda.is_available():
        raise SystemExit("diag_fps_tiled: needs a GPU (no timing without one)")
    xyz = torch.from_numpy((box_surface_cloud(np.random.default_rng(N), N, (0.3, 0.2, 0.1)) + 0.25).astype(np.float32)[None]).cuda()
    idx = torch.empty(1, M, dtype=torch.int32, device="cuda")
    new_xyz = torch.empty(1, M, 3, device="cuda")
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        dev, host = [], []
        for _ in range(rounds):
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e6)
            b.record()
            torch.cuda.synchronize()
            dev.append(a.elapsed_time(b) * 1e3)
        return np.median(dev), min(dev), max(dev), np.median(host)

    print("N %d M %d B 1 on %s (%d rounds; us)" % (N, M, torch.cuda.get_device_name(0), rounds))
    ref = None
    if N == 8192:
        d, lo, hi, h = timed(lambda: hip.call("gad_furthest_point_sampling", xyz, 1, N, M, idx, new_xyz))
        ref = idx.clone()
        print("  LDS kernel (one workgroup)        call %9.1f (min %9.1f max %9.1f)   per round %7.2f   enqueue %8.1f" % (d, lo, hi, d / M, h))
    for slice_ in SLICES:
        groups = (N + slice_ - 1) // slice_
        ws = torch.empty(hip.lib().gad_fps_tiled_workspace_bytes(1, N, M, groups), dtype=torch.uint8, device="cuda")
        d, lo, hi, h = timed(lambda: hip.call("gad_fps_tiled", xyz, 1, N, M, groups, idx, new_xyz, ws))
        if ref is None:
            ref = idx.clone()
        same = bool((idx == ref).all())
        per = d / (M + 1)
        print("  tiled slice %5d groups %4d      call %9.1f (min %9.1f max %9.1f)   per round %7.2f   %5.2f %% of the HBM peak   "
              "enqueue %8.1f (%.2f per launch)   indices equal to the first row's: %s"
              % (slice_, groups, d, lo, hi, per, 100.0 * N * 20 / (per * 1e-6) / HBM_PEAK, h, h / (M + 1), same))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_tiled.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rounds)
        return 0
    lines = ["gad_fps_tiled, one launch per pick: time per round by cloud size and slice size (points per workgroup)",
             "command: python tools/diag_fps_tiled.py --rounds %d" % a.rounds,
             "device events around one call after one warm-up call, median over the rounds; per round = call / (M + 1) launches; "
             "bytes per round = N x 20 against an HBM peak of %.1f TB/s" % (HBM_PEAK / 1e12)]
    rc = 0
    for N in SIZES:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--child", str(N)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines.append(p.stdout.rstrip())
        print(p.stdout, end="")
        sys.stdout.flush()
        if p.returncode != 0:
            rc = p.returncode
            lines.append("N %d: the child ended with status %d -- stopped here" % (N, rc))
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
