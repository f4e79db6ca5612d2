"""Prints one sha256 per stand-alone set-abstraction module case (tools/dump_launch_lists.py MODULE_CASES, without the
coordinate-gradient ones: those are refused in deterministic mode) over what one training forward + backward and one eval forward
compute in the library's deterministic mode: new_xyz, the output, the eval output, features.grad, every parameter's .grad and the
BatchNorm running statistics.  Seeded inputs and weights, so two trees on the same box compare digest for digest: a launch list
may be item-identical (dump_launch_lists.py) and still name another buffer -- that moves a digest.

    python tools/digest_sa_module.py [--out digest.txt]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def digest(kw, B, N):
    from tools.dump_launch_lists import build_module, module_inputs, run_module
    mod = build_module(kw)
    new_xyz, out, out_eval, _, feats = run_module(mod, *module_inputs(kw, B, N))
    h = hashlib.sha256()
    named = [("new_xyz", new_xyz), ("out", out), ("out_eval", out_eval), ("features.grad", feats.grad)]
    named += [("grad " + n, p.grad) for n, p in mod.named_parameters()]
    named += [(n, t) for n, t in mod.state_dict().items() if "running" in n or "num_batches" in n]
    for name, t in named:
        h.update(name.encode())
        if t is not None:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest(), len(named)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ga_ddpg_amd import hip
    from tools.dump_launch_lists import MODULE_CASES
    if not torch.cuda.is_available():
        raise SystemExit("digest_sa_module: needs a GPU")
    hip.set_option("deterministic", 1)
    lines = []
    for name, kw, B, N in MODULE_CASES:
        try:
            d, n = digest(kw, B, N)
            lines.append("%-16s B %d N %4d  %3d tensors  sha256 %s" % (name, B, N, n, d))
        except RuntimeError as e:              # (a shape an entry point refuses: the same words on both trees)
            lines.append("%-16s B %d N %4d  refused: %s" % (name, B, N, e))
        print(lines[-1])
        sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
