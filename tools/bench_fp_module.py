"""What PointnetFPModule's `fused` switch costs or saves: forward + backward in train mode, the fused path (ga_ddpg_amd.fp_function:
one row matrix, the layer GEMMs, BatchNorm statistics in their epilogues) against the composition (three_interpolate, torch.cat,
Conv2d / BatchNorm2d / ReLU as torch modules), on the four decoder levels of a PointNet++ SSG segmentation network over
4096-point clouds at B = 16:

    (n, m, mlp) = (64, 16, [768, 256, 256]), (256, 64, [384, 256, 256]), (1024, 256, [320, 256, 128]),
                  (4096, 1024, [128 + 6, 128, 128, 128])

known_feats carries two thirds of mlp[0] at the three coarse levels (the coarser level's output) and 128 at the finest, the skip
features the rest.  Both modules hold the same weights.  After `--warmup` calls of each, the two legs alternate within a round;
a leg is `--calls` back-to-back forward + backward calls between two device events; the table gives the median over `--rounds`
rounds and their spread, in microseconds per call.  Also printed: the largest relative difference of the two forward outputs
(relative to the largest composed value).  Not collected by pytest, not part of bench.py; no threshold or route depends on it.

    python tools/bench_fp_module.py --out profiles/fp_fused.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEVELS = ((64, 16, [768, 256, 256], 512), (256, 64, [384, 256, 256], 256), (1024, 256, [320, 256, 128], 256),
          (4096, 1024, [128 + 6, 128, 128, 128], 128))          # (n, m, mlp, C2)


def leg(mod, args, G, calls):
    unknown, known, uf, kf = args
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        mod.zero_grad(set_to_none=True)
        uf.grad = kf.grad = None
        (mod(unknown, known, uf, kf) * G).sum().backward()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1000.0 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ga_ddpg_amd  # noqa: F401
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    B = a.batch
    lines = ["PointnetFPModule forward + backward (train mode): fused=True (fp_function: row matrix + layer GEMMs) against the composition",
             "command: python tools/bench_fp_module.py " + " ".join(sys.argv[1:]),
             "device events around %d back-to-back forward + backward calls after %d warm-up calls of each leg; legs alternate within "
             "a round; %d rounds; us per call" % (a.calls, a.warmup, a.rounds),
             "device: %s; one process; B = %d; library options %s" % (torch.cuda.get_device_name(0), B,
                                                                      {k: hip.get_option(k) for k in ("mfma_split", "deterministic")})]
    for n, m, spec, c2 in LEVELS:
        torch.manual_seed(n)
        c1 = spec[0] - c2
        mods = {"composed": PointnetFPModule(spec).cuda().train(), "fused": PointnetFPModule(spec, fused=True).cuda().train()}
        mods["fused"].load_state_dict(mods["composed"].state_dict())
        unknown, known = torch.rand(B, n, 3, device="cuda"), torch.rand(B, m, 3, device="cuda")
        uf = torch.randn(B, c1, n, device="cuda", requires_grad=True)
        kf = torch.randn(B, c2, m, device="cuda", requires_grad=True)
        G = torch.randn(B, spec[-1], n, device="cuda")
        args = (unknown, known, uf, kf)
        with torch.no_grad():
            y = {k: mod(*args) for k, mod in mods.items()}
        assert mods["fused"].last_route == "fused" and mods["composed"].last_route == "composed"
        diff = float((y["fused"] - y["composed"]).abs().max() / y["composed"].abs().max())
        for mod in mods.values():
            leg(mod, args, G, a.warmup)
        t = {k: [] for k in mods}
        for _ in range(a.rounds):
            for k in ("composed", "fused"):
                t[k].append(leg(mods[k], args, G, a.calls))
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append("level n %4d m %4d mlp %-22s C2 %3d  (max |fused - composed| / max |composed| of the forward output %.2e)"
                     % (n, m, spec, c2, diff))
        for k in ("composed", "fused"):
            lines.append("  %-9s %9.1f us (min %9.1f max %9.1f)" % (k, med[k], min(t[k]), max(t[k])))
        lines.append("  composed / fused %.2f" % (med["composed"] / med["fused"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
