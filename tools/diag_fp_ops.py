"""Times gad_three_nn, gad_three_interpolate and gad_three_interpolate_grad (through pointnet2_utils) against the composition a
user would otherwise write in torch on the same GPU: torch.cdist(...)**2 + topk(3, largest=False); gather + weighted sum; autograd
of that.  Recorded, not gated (the correctness gates are tests/test_gpu_fp_ops.py).

    python tools/diag_fp_ops.py [--out profiles/fp_ops.txt] [--rounds 5]

Every shape runs in a child process of its own under a time limit; the first child that fails or runs out of time ends the run.
Times are device events around `iters` back-to-back calls after a warm-up, the two legs alternating within a round; the table
gives the median over the rounds with min and max."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((64, 4096, 1024, 128), (64, 1024, 256, 256), (1, 1024, 256, 256))       # (B, n, m, C)
CHILD_LIMIT = 300                                                                 # seconds per shape


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


def child(B, n, m, C_, rounds):
    import numpy as np
    import torch
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    if not torch.cuda.is_available():
        raise SystemExit("diag_fp_ops: needs a GPU (no timing without one)")
    g = torch.Generator(device="cuda").manual_seed(B * 7 + n)
    unknown = torch.rand(B, n, 3, device="cuda", generator=g)
    known = torch.rand(B, m, 3, device="cuda", generator=g)
    feats = torch.randn(B, C_, m, device="cuda", generator=g).requires_grad_(True)
    gout = torch.randn(B, C_, n, device="cuda", generator=g)
    dist, idx = pu.three_nn(unknown, known)
    w = 1.0 / (dist + 1e-8)
    w = w / w.sum(2, keepdim=True)
    idx64 = idx.long()

    def torch_nn():
        d2 = torch.cdist(unknown, known) ** 2
        return torch.topk(d2, 3, dim=2, largest=False)

    def torch_interp(f):
        nb = torch.gather(f, 2, idx64.reshape(B, 1, n * 3).expand(B, C_, n * 3)).reshape(B, C_, n, 3)
        return (nb * w.unsqueeze(1)).sum(-1)

    def hip_grad():
        feats.grad = None
        out_h.backward(gout, retain_graph=True)

    def torch_grad():
        feats.grad = None
        out_t.backward(gout, retain_graph=True)

    out_h, out_t = pu.three_interpolate(feats, idx, w), torch_interp(feats)
    agree = float((torch_nn()[1] == idx64).float().mean()) if m >= 3 else float("nan")
    diff = float((out_h - out_t).detach().abs().max())
    legs = (("three_nn", lambda: pu.three_nn(unknown, known), torch_nn),
            ("three_interpolate", lambda: pu.three_interpolate(feats.detach(), idx, w), lambda: torch_interp(feats.detach())),
            ("three_interpolate_grad", hip_grad, torch_grad))
    work = B * n * m
    iters = 200 if work < (1 << 24) else (50 if work < (1 << 27) else 20)
    print("shape B %d n %d m %d C %d on %s   (%d calls per timed window, %d rounds; neighbour indices equal to torch's on %.4f of the "
          "slots; max |interpolation - torch| %.2e)" % (B, n, m, C_, torch.cuda.get_device_name(0), iters, rounds, agree, diff))
    for name, hip_fn, torch_fn in legs:
        th, tt = [], []
        for _ in range(rounds):
            th.append(_time(hip_fn, iters))
            tt.append(_time(torch_fn, iters))
        print("  %-24s libgaddpg %9.1f us (min %9.1f max %9.1f)   torch %9.1f us (min %9.1f max %9.1f)   torch / libgaddpg %6.2f"
              % (name, np.median(th), min(th), max(th), np.median(tt), min(tt), max(tt), np.median(tt) / np.median(th)))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp_ops.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", type=int, nargs=4, default=None)
    a = ap.parse_args()
    if a.child:
        child(*a.child, rounds=a.rounds)
        return 0
    lines = ["three_nn / three_interpolate / three_interpolate_grad against the torch composition (cdist**2 + topk; gather + weighted "
             "sum; autograd of that)",
             "command: python tools/diag_fp_ops.py --rounds %d" % a.rounds,
             "device events around back-to-back calls after 3 warm-up calls; legs alternate within a round; us per call"]
    rc = 0
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds), "--child"]
        p = subprocess.run(cmd + [str(x) for x in shape], stdout=subprocess.PIPE, text=True)
        lines.append(p.stdout.rstrip())
        print(p.stdout, end="")
        sys.stdout.flush()
        if p.returncode != 0:
            rc = p.returncode
            lines.append("shape %s: the child ended with status %d -- stopped here" % (shape, rc))
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
