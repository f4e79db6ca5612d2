"""Are the kernels of two csrc directories the same device code?  For a refactor that moves kernels between units.
usage: python tools/compare_device_code.py PARENT_CSRC TREE_CSRC [--parent-units U ...] [--tree-units U ...] [--work DIR] [--jobs N]
(CPU-only host.  U: unit names or glob patterns inside that side's csrc, e.g. --parent-units geometry.hip --tree-units fps.hip
ball_query.hip group.hip interpolate.hip library.hip, or 'gemm*.hip' for both; the default is every *.hip of the side)

Each unit is compiled once with the Makefile's FLAGS plus --offload-device-only -S -Rpass-analysis=kernel-resource-usage.  The assembly
is cut at the kernel symbols (.amdhsa_kernel), comments and directives are dropped, basic-block labels are renumbered in order of
appearance, and the text that is left is compared kernel by kernel; the remarks give VGPRs, AGPRs, spills, LDS, scratch and occupancy.
Exit status 0: the same kernel symbols, each in exactly one unit, every one identical in instructions and resources."""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

RESOURCES = ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


def make_var(csrc, var):
    out = subprocess.check_output(["make", "-s", "-C", csrc, "--no-print-directory", "--eval", "print-var: ; @echo $(%s)" % var, "print-var"])
    return out.decode().split()


def compile_unit(csrc, unit, work):
    base = os.path.join(work, unit[:-4])
    cmd = make_var(csrc, "HIPCC") + make_var(csrc, "FLAGS") + ["--offload-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", unit, "-o", base + ".s"]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=csrc, stderr=subprocess.PIPE)
    if r.returncode:
        sys.exit("%s: %s failed\n%s" % (csrc, unit, r.stderr.decode()[-4000:]))
    open(base + ".log", "w").write(r.stderr.decode())
    return unit, open(base + ".s").read(), r.stderr.decode(), time.time() - t0


def kernels_of(asm):
    """{kernel symbol: [instruction and label lines]}"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out, cur, labels = {}, None, {}
    for line in asm.split("\n"):
        s = line.split(";")[0].strip()
        if not s:
            continue
        if s.endswith(":") and s[:-1] in names:
            cur, labels = out.setdefault(s[:-1], []), {}
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".") and not s.endswith(":"):
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), s))
    return out


def resources_of(log):
    """The remarks' figures per mangled name.  (tools/kernel_resources.py reads the same remarks, but is a script that prints five of
    them under demangled, truncated names: nothing there to import, and the spill counts are needed here.)"""
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", log)[1:]:
        out[b.split()[0]] = tuple((re.search(re.escape(k) + r": (\d+)", b) or [None, "?"])[1] for k in RESOURCES)
    return out


def side(csrc, patterns, work, jobs):
    os.makedirs(work, exist_ok=True)
    units = sorted({os.path.basename(p) for pat in patterns for p in glob.glob(os.path.join(csrc, pat))})
    if not units:
        sys.exit("%s: no unit matches %s" % (csrc, " ".join(patterns)))
    code, res, where = {}, {}, {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for unit, asm, log, secs in ex.map(lambda u: compile_unit(csrc, u, work), units):
            ks = kernels_of(asm)
            print("  %-16s %3d kernel symbols, %6d instructions  (%.0f s)" % (unit, len(ks), sum(len(v) for v in ks.values()), secs))
            for k, v in ks.items():
                where.setdefault(k, []).append(unit)
                code[k] = v
            res.update(resources_of(log))
    return code, res, where


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--parent-units", nargs="+", default=["*.hip"], metavar="U", help="units of the parent to compile (names or patterns)")
    ap.add_argument("--tree-units", nargs="+", default=["*.hip"], metavar="U", help="units of the tree to compile")
    ap.add_argument("--work", default=None, help="where the .s files go (default: a temporary directory)")
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix="cmpdev_")
    sides = []
    for tag, csrc, units in (("parent", a.parent, a.parent_units), ("tree", a.tree, a.tree_units)):
        print("%s: %s" % (tag, csrc))
        sides.append(side(os.path.abspath(csrc), units, os.path.join(work, tag), a.jobs))
    (pc, pr, pw), (tc, tr, tw) = sides
    bad = 0
    for tag, w in (("parent", pw), ("tree", tw)):
        for k, us in sorted(w.items()):
            if len(us) > 1:
                bad += 1
                print("IN MORE THAN ONE UNIT (%s): %s  %s" % (tag, k, us))
    missing, new = sorted(set(pc) - set(tc)), sorted(set(tc) - set(pc))
    for k in missing:
        print("MISSING in the tree: %s (parent: %s)" % (k, pw[k][0]))
    for k in new:
        print("NEW in the tree: %s (%s)" % (k, tw[k][0]))
    same = diff_code = diff_res = 0
    for k in sorted(set(pc) & set(tc)):
        if pc[k] != tc[k]:
            diff_code += 1
            d = [l for l in difflib.unified_diff(pc[k], tc[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print("DIFFERENT %s (%s -> %s): %d -> %d instructions, %d diff lines" % (k, pw[k][0], tw[k][0], len(pc[k]), len(tc[k]), len(d)))
            for l in d[:6]:
                print("    " + l)
        else:
            same += 1
        if pr.get(k) != tr.get(k) or k not in pr:
            diff_res += 1
            print("RESOURCES %s: %s" % (k, ", ".join("%s %s -> %s" % (n, x, y) for n, x, y in zip(RESOURCES, pr.get(k, "?" * 7), tr.get(k, "?" * 7)) if x != y)))
    print("kernel symbols: parent %d, tree %d; missing %d, new %d, in more than one unit %d" % (len(pc), len(tc), len(missing), len(new), bad))
    print("instructions compared: %d" % sum(len(pc[k]) for k in set(pc) & set(tc)))
    print("identical: %d of %d; resource figures (%s) equal: %d of %d" % (same, len(pc), " / ".join(RESOURCES), len(set(pc) & set(tc)) - diff_res, len(pc)))
    sys.exit(1 if bad or missing or new or diff_code or diff_res else 0)


if __name__ == "__main__":
    main()
