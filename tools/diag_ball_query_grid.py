"""Times gad_ball_query -- beyond 4096 points the scan: one wavefront per centroid walks the cloud -- against gad_ball_query_grid
(uniform grid in global memory, include/gaddpg.h section A) on the same seeded inputs.  Recorded, not gated (the correctness gates
are tests/test_gpu_ball_query_grid.py); the routing rule of pointnet2_utils.ball_query_uses_grid is taken from this table.

    python tools/diag_ball_query_grid.py [--out profiles/ball_query_grid.txt] [--rounds 5]

B = 1 box-surface cloud (synth_data.box_surface_cloud, edges 0.3 x 0.2 x 0.1) of N points; M centroids drawn from the cloud
(seeded; with replacement where M > N); two radii, sized so that a ball on a face holds about 16 and about 300 points; nsample 32
and 64.  Per row the two entry points alternate inside one process: after a warm-up call of each, `rounds` windows per entry
point, scan window / grid window / scan window ..., every window between two device events and long enough (repetitions chosen
from the warm-up) that it is milliseconds, not microseconds.  A row prints the median time per call of each, the min .. max over
its windows (the run-to-run spread), the ratio of the medians -- and only after idx and cnt of the two were compared equal.
Every N runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the run."""
import argparse
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (4097, 8192, 65536, 262144, 1048576)
CENTROIDS = (1024, 4096, 16384)
BALLS = (16, 300)                        # points a ball on a face holds
NSAMPLES = (32, 64)
EDGES = (0.3, 0.2, 0.1)
AREA = 2.0 * (EDGES[0] * EDGES[1] + EDGES[0] * EDGES[2] + EDGES[1] * EDGES[2])
WINDOW_US = 4000.0                       # least length of a timed window
CHILD_LIMIT = 150                        # seconds per N


def child(N, rounds):
    import numpy as np
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.synth_data import box_surface_cloud
    if not torch.cuda.is_available():
        raise SystemExit("diag_ball_query_grid: needs a GPU (no timing without one)")
    rng = np.random.default_rng(N)
    cloud = (box_surface_cloud(rng, N, EDGES) + 0.25).astype(np.float32)
    xyz = torch.from_numpy(cloud[None]).cuda()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    print("N %d B 1 on %s (%d windows per entry point; us per call: median (min .. max))" % (N, torch.cuda.get_device_name(0), rounds))
    for M in CENTROIDS:
        ctr = torch.from_numpy(cloud[rng.choice(N, size=M, replace=M > N)][None]).cuda()
        for ball in BALLS:
            radius = math.sqrt(ball * AREA / (math.pi * N))
            for S in NSAMPLES:
                out = [(torch.empty(1, M, S, dtype=torch.int32, device="cuda"), torch.empty(1, M, dtype=torch.int32, device="cuda"))
                       for _ in range(2)]
                ws = hip.workspace("gad_ball_query_grid", "cuda", 1, N, M, S)
                scan = lambda: hip.call("gad_ball_query", ctr, xyz, 1, N, M, radius, S, out[0][0], out[0][1])
                grid = lambda: hip.call("gad_ball_query_grid", ctr, xyz, 1, N, M, radius, S, out[1][0], out[1][1], ws)
                reps = []
                for fn in (scan, grid):
                    window(fn, 1)                                  # warm-up
                    reps.append(int(min(400, max(3, math.ceil(WINDOW_US / max(window(fn, 2), 1.0))))))
                assert bool((out[0][0] == out[1][0]).all()) and bool((out[0][1] == out[1][1]).all()), "outputs differ"
                t = ([], [])
                for _ in range(rounds):
                    t[0].append(window(scan, reps[0]))
                    t[1].append(window(grid, reps[1]))
                ms, mg = float(np.median(t[0])), float(np.median(t[1]))
                print("  M %5d  radius %.5f (~%3d points, mean count %5.1f)  nsample %2d   scan %9.1f (%9.1f .. %9.1f) x%-3d   "
                      "grid %8.1f (%8.1f .. %8.1f) x%-3d   scan / grid %6.2f   outputs equal"
                      % (M, radius, ball, float(out[0][1].float().mean()), S, ms, min(t[0]), max(t[0]), reps[0], mg, min(t[1]),
                         max(t[1]), reps[1], ms / mg))
                sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ball_query_grid.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rounds)
        return 0
    lines = ["gad_ball_query (the scan beyond 4096 points) against gad_ball_query_grid: time per call by cloud size, centroids, radius "
             "and nsample",
             "command: python tools/diag_ball_query_grid.py --rounds %d" % a.rounds,
             "the two entry points alternate window by window in one process; a window is x<repetitions> calls between two device "
             "events, at least %.0f ms long unless 400 calls are shorter; outputs compared equal before a row is printed"
             % (WINDOW_US / 1e3)]
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
