"""Times gad_three_nn -- exhaustive: every query lane walks all m known points through LDS tiles -- against gad_three_nn_grid
(uniform grid over the known points in global memory, searched ring by ring; include/gaddpg.h section A) on the same seeded
inputs.  Recorded, not gated (the correctness gates are tests/test_gpu_three_nn_grid.py); the routing rule of
pointnet2_utils.three_nn_uses_grid is taken from this table.

    python tools/diag_three_nn_grid.py [--out profiles/three_nn_grid.txt] [--rounds 5]

B = 1 and B = 8 clouds of m known points, m from 2048 to 1 048 576 in steps of 2 x, with n = m / 4, m and 4 m queries; box-surface
clouds (synth_data.box_surface_cloud, edges 0.3 x 0.2 x 0.1) and uniform-cube clouds, the queries drawn from the same
distribution as the known points (independently), and "outside": the uniform cube with queries from a cube 1.5 x as wide
around it (70 % of them outside the box of the known points: the regime of the exhaustive fallback).  The exhaustive call is timed where B * n * m <= 1e11 distance evaluations
(about 50 ms at the 2.3e12 evaluations per second of profiles/fp_ops.txt); beyond that the row holds the grid alone.  Per row
the two entry points alternate inside one process: after a warm-up call of each, `rounds` windows per entry point, exhaustive
window / grid window / exhaustive window ..., every window between two device events and long enough (repetitions chosen from
the warm-up) that it is milliseconds, not microseconds.  A row prints the median time per call of each, the min .. max over its
windows (the run-to-run spread), the ratio of the medians and the share of the queries the grid call redid exhaustively (its
`stats`) -- and only after dist2 and idx of the two were compared equal.  A row counts for the grid if its slowest grid window is
faster than the fastest exhaustive window.  Every m runs in a child process of its own under a time limit; the first child that
fails or runs out of time ends the run.  The last lines name the smallest measured m from which the grid wins every row."""
import argparse
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = tuple(2048 << k for k in range(10))          # 2048 .. 1 048 576
BATCHES = (1, 8)
CLOUDS = ("surface", "cube", "outside")
EDGES = (0.3, 0.2, 0.1)
EXHAUSTIVE_MAX_EVALS = 1.0e11            # B * n * m beyond which gad_three_nn is not timed (about 50 ms)
WINDOW_US = 4000.0                       # least length of a timed window
CHILD_LIMIT = 240                        # seconds per m


def child(m, rounds):
    import numpy as np
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.synth_data import box_surface_cloud
    if not torch.cuda.is_available():
        raise SystemExit("diag_three_nn_grid: needs a GPU (no timing without one)")
    rng = np.random.default_rng(m)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def cloud(kind, B, k, queries=False):
        if kind == "surface":
            return np.stack([box_surface_cloud(rng, k, EDGES) + 0.25 for _ in range(B)]).astype(np.float32)
        if kind == "outside" and queries:
            return (0.1 + (rng.random((B, k, 3)) * 1.5 - 0.25) * 0.4).astype(np.float32)
        return (rng.random((B, k, 3)) * 0.4 + 0.1).astype(np.float32)

    def window(fn, reps):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    def timed(fn):
        window(fn, 1)                                          # warm-up
        return int(min(400, max(3, math.ceil(WINDOW_US / max(window(fn, 2), 1.0)))))

    print("m %d on %s (%d windows per entry point; us per call: median (min .. max))" % (m, torch.cuda.get_device_name(0), rounds))
    rows = wins = 0
    for kind in CLOUDS:
        for B in BATCHES:
            known = torch.from_numpy(cloud(kind, B, m)).cuda()
            for n in (m // 4, m, 4 * m):
                unknown = torch.from_numpy(cloud(kind, B, n, True)).cuda()
                out = [(torch.empty(B, n, 3, dtype=torch.float32, device="cuda"), torch.empty(B, n, 3, dtype=torch.int32, device="cuda"))
                       for _ in range(2)]
                stats = torch.empty(B, 2, dtype=torch.int32, device="cuda")
                ws = hip.workspace("gad_three_nn_grid", "cuda", B, n, m)
                exhaustive = lambda: hip.call("gad_three_nn", unknown, known, B, n, m, out[0][0], out[0][1])
                grid = lambda: hip.call("gad_three_nn_grid", unknown, known, B, n, m, out[1][0], out[1][1], None, ws)
                hip.call("gad_three_nn_grid", unknown, known, B, n, m, out[1][0], out[1][1], stats, ws)
                redone = float(stats[:, 1].sum().item()) / float(B * n)
                both = float(B) * n * m <= EXHAUSTIVE_MAX_EVALS
                head = "  %-7s B %d  n %8d" % (kind, B, n)
                rg = timed(grid)
                if both:
                    re_ = timed(exhaustive)
                    assert bool((out[0][1] == out[1][1]).all()) and bool((out[0][0].view(torch.int32) == out[1][0].view(torch.int32)).all()), \
                        "outputs differ"
                t = ([], [])
                for _ in range(rounds):
                    if both:
                        t[0].append(window(exhaustive, re_))
                    t[1].append(window(grid, rg))
                mg = float(np.median(t[1]))
                tail = "grid %9.1f (%9.1f .. %9.1f) x%-3d   redone exhaustively %6.2f %%" % (mg, min(t[1]), max(t[1]), rg, 100.0 * redone)
                if both:
                    me = float(np.median(t[0]))
                    win = max(t[1]) < min(t[0])
                    rows, wins = rows + 1, wins + int(win)
                    print("%s   exhaustive %10.1f (%10.1f .. %10.1f) x%-3d   %s   exhaustive / grid %7.2f   outputs equal   %s"
                          % (head, me, min(t[0]), max(t[0]), re_, tail, me / mg, "grid faster" if win else "grid NOT faster"))
                else:
                    print("%s   exhaustive   not timed (B * n * m > %.0e)%s   %s" % (head, EXHAUSTIVE_MAX_EVALS, " " * 13, tail))
                sys.stdout.flush()
    print("VERDICT m %d: grid faster beyond the spread in %d of %d rows with both timed" % (m, wins, rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "three_nn_grid.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rounds)
        return 0
    lines = ["gad_three_nn (exhaustive) against gad_three_nn_grid: time per call by known points m, queries n, clouds B and distribution",
             "command: python tools/diag_three_nn_grid.py --rounds %d" % a.rounds,
             "the two entry points alternate window by window in one process; a window is x<repetitions> calls between two device "
             "events, at least %.0f ms long unless 400 calls are shorter; outputs compared equal before a row is printed; the grid "
             "call includes building the grid (seven launches) and is timed with stats = NULL" % (WINDOW_US / 1e3)]
    rc, verdicts = 0, {}
    for m in SIZES:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--child", str(m)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines.append(p.stdout.rstrip())
        print(p.stdout, end="")
        sys.stdout.flush()
        if p.returncode != 0:
            rc = p.returncode
            lines.append("m %d: the child ended with status %d -- stopped here" % (m, rc))
            break
        v = re.search(r"VERDICT m (\d+): .* in (\d+) of (\d+) rows", p.stdout)
        verdicts[int(v.group(1))] = (int(v.group(2)), int(v.group(3)))
    # the rule: the smallest measured m from which every m with timed rows has the grid ahead in all of them
    first = None
    for m in sorted(verdicts, reverse=True):
        wins, rows = verdicts[m]
        if rows and wins < rows:
            break
        if rows:
            first = m
    lines.append("rule: " + ("the grid is faster than gad_three_nn beyond the spread in every timed row from m = %d" % first
                             if first is not None and rc == 0 else "no measured m from which the grid wins every timed row"))
    print(lines[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
