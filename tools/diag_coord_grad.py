"""Times the coordinate gradient of the fused set-abstraction path (module switch `coordinate_grad`, entry point gad_sa_coord_grad)
at B 64 and B 1, N 1024, npoint 128, nsample 64, mlp [4, 64, 64, 128]:

  - the two launches of gad_sa_coord_grad alone, on the buffers a real backward left behind, with the bytes they move
    (G and z of every live row once, the row lists, three float atomics per row) against the HBM peak;
  - the module's forward + backward with the switch off and on;
  - forward + backward of the same module through _generic_forward (upstream's composition over the section A operators),
    the only other way this package gives these gradients.

Recorded, not gated (the correctness gates are tests/test_gpu_coord_grad.py); nothing routes on these numbers.

    python tools/diag_coord_grad.py [--out profiles/coord_grad.txt] [--rounds 7]

Every shape runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the run.
Times are device events around `iters` back-to-back calls after a warm-up, the legs alternating within a round; the table gives
the median over the rounds with min and max."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = (64, 1)                     # B
N, NPOINT, NSAMPLE, RADIUS, MLP = 1024, 128, 64, 0.1, [4, 64, 64, 128]
CHILD_LIMIT = 240                    # seconds per shape
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12          # bytes / s (float4 copy; datasheet)


def _time(fn, iters, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                        # us per call


def child(B, rounds):
    import ctypes as C
    import numpy as np
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    if not torch.cuda.is_available():
        raise SystemExit("diag_coord_grad: needs a GPU (no timing without one)")
    torch.manual_seed(B)
    kw = dict(mlp=list(MLP), npoint=NPOINT, radius=RADIUS, nsample=NSAMPLE)
    mods = {"off": pm.PointnetSAModule(**kw).cuda().train(), "on": pm.PointnetSAModule(coordinate_grad=True, **kw).cuda().train()}
    mods["on"].load_state_dict(mods["off"].state_dict())
    g = torch.Generator(device="cuda").manual_seed(B * 7 + N)
    xyz = (torch.rand(B, N, 3, device="cuda", generator=g) * 0.5).requires_grad_(True)
    feats = torch.randn(B, MLP[0], N, device="cuda", generator=g).requires_grad_(True)
    probe = torch.randn(B, MLP[-1], NPOINT, device="cuda", generator=g)
    probe2 = torch.randn(B, NPOINT, 3, device="cuda", generator=g)

    def step(forward):
        def run():
            xyz.grad = feats.grad = None
            new_xyz, out = forward(xyz, feats)
            loss = (out * probe).sum()
            if new_xyz.requires_grad:
                loss = loss + (new_xyz * probe2).sum()
            loss.backward()
        return run
    legs = (("fused, switch off", step(mods["off"])), ("fused, switch on", step(mods["on"])),
            ("_generic_forward", step(mods["on"]._generic_forward)))
    # agreement of the two ways to these gradients before anything is timed
    legs[1][1]()
    gx_fused = xyz.grad.clone()
    legs[2][1]()
    gx_generic = xyz.grad.clone()
    err = (gx_fused - gx_generic).abs() / gx_generic.abs().max()
    diff, n_off = float(err.max()), int((err > 1e-4).sum())           # (a max-pool or ReLU decision that rounds the other way moves a whole term)
    # the new call alone: the plan item of the run the backward above recycled, on the buffers it left
    net = mods["on"]._gad_rt["net"]
    run = net.free[(B, N)][0]
    item = [it for it in run.bwd_xyz.calls if it.kind == "call" and it.name == "gad_sa_coord_grad"][0]
    argv = [C.byref(x) if isinstance(x, C.Structure) else x for x in item.argv]

    def alone():
        hip.check(item.f(*(argv + [hip.stream()])), item.name)
    rows = int(run.rows["n"].item())
    n_out = MLP[1]
    read = rows * (2 * n_out * 4 + 12)                  # G and z of the row, row_w / row_pt / row_grp
    atom = rows * 3 * 4 + B * NPOINT * 3 * 4 * 2        # three adds per row on dxyz, the run sums on dctr (at least one per group), the centroids
    iters = 20 if B > 1 else 100
    print("B %d N %d npoint %d nsample %d mlp %s on %s: %d live rows of %d (%d calls per timed window, %d rounds); "
          "max |d xyz fused - generic| / max |generic| %.2e, %d of %d elements beyond 1e-4"
          % (B, N, NPOINT, NSAMPLE, MLP, torch.cuda.get_device_name(0), rows, run.rows["cap"], iters, rounds, diff, n_off, err.numel()))
    times = {name: [] for name, _ in legs}
    t_alone = []
    for _ in range(rounds):
        t_alone.append(_time(alone, iters * 5))
        for name, fn in legs:
            times[name].append(_time(fn, iters))
    ta = float(np.median(t_alone))
    print("  gad_sa_coord_grad alone (2 launches) %9.1f us (min %9.1f max %9.1f): reads %.2f MB + %.2f MB of float atomics; reads / time = "
          "%.2f TB/s = %.1f %% of the measured HBM peak (6.29 TB/s), %.1f %% of the datasheet's 8 TB/s"
          % (ta, min(t_alone), max(t_alone), read / 1e6, atom / 1e6, read / ta / 1e6, 100 * read / (ta * 1e-6) / HBM_MEASURED,
             100 * read / (ta * 1e-6) / HBM_SPEC))
    for name, _ in legs:
        t = times[name]
        print("  forward + backward, %-20s %9.1f us (min %9.1f max %9.1f)" % (name, np.median(t), min(t), max(t)))
    on, off, gen = (float(np.median(times[k])) for k in ("fused, switch on", "fused, switch off", "_generic_forward"))
    print("  switch on - off %+.1f us (%.1f %% of the switch-off step); _generic_forward / fused switch on %.2f%s"
          % (on - off, 100 * (on - off) / off, gen / on, "" if gen >= on else "   <-- the fused path with the switch on is SLOWER here"))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coord_grad.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, rounds=a.rounds)
        return 0
    lines = ["coordinate gradient of the fused set-abstraction path: gad_sa_coord_grad alone; module forward + backward with the switch "
             "off / on; the same through _generic_forward",
             "command: python tools/diag_coord_grad.py --rounds %d" % a.rounds,
             "device events around back-to-back calls after 3 warm-up calls; legs alternate within a round; us per call, median (min, max)"]
    rc = 0
    for B in SHAPES:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--child", str(B)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines.append(p.stdout.rstrip())
        print(p.stdout, end="")
        sys.stdout.flush()
        if p.returncode != 0:
            rc = p.returncode
            lines.append("B %d: the child ended with status %d -- stopped here" % (B, rc))
            break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
